"""RISE on the device: the kernels of csrc/rise.hip on their own (through _lib.call with raw pointers) against the host Philox
model, the float32 twin formula (bit for bit) and the fp64 map of tests/_rise_inputs.py; their refusals; rise against the
model's own forward on batches the test builds itself with rise_apply_torch (bit for bit), with and without encoder reuse;
rise against rise_torch; the remaining options.

Every buffer of the kernel tests lives in the Arena of tests/test_gpu_bn_reduce.py: bytes outside the outputs (the inputs
included) must be unchanged, every output element written."""
import pytest
import torch

import _rise_inputs as ri
from _golden import Golden
from oracle import params as P
from test_gpu_bn_reduce import Arena, _call, _st
from test_gpu_model import DEV, build
from test_host_rise import Cube, cube_volumes

pytestmark = pytest.mark.gpu
F32, F64, U8, I32 = torch.float32, torch.float64, torch.uint8, torch.int32


def _byte_slot(n):
    """An Arena output of n bytes: the Arena judges 2- and 4-byte words, so the slot is int32 words (nodes are 0 / 1: a written
    word is never the fill pattern)."""
    return ((-(-n // 4),), I32)


def _bytes(words, shape):
    """The n bytes of such a slot -> uint8 of `shape`; the bytes behind them in the last word still hold the fill pattern."""
    b, n = words.view(U8), 1
    for d in shape:
        n *= d
    assert bool((b[n:] == 0xFF).all()), "bytes behind the node grids were written"
    return b[:n].view(shape)


# ---------------------------------------------------------------------------------------------------------------------
# the kernels through raw pointers
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("geom", ri.GEOMETRIES, ids=ri.geom_id)
def test_masks_kernel_equals_the_philox_model(geom):
    """Byte for byte, for three seeds (one above 2^32) and for m0 > 0: the second call draws masks 4 .. MASKS-1 on their own."""
    size, cells = geom
    _cell, nn, _G = ri.geometry(size, cells)
    N = ri.MASKS
    outs = {}
    for i in range(len(ri.SEEDS)):
        outs[f"nodes{i}"], outs[f"shifts{i}"] = _byte_slot(N * _G), ((N, 3), I32)
    outs["late_nodes"], outs["late_shifts"] = _byte_slot((N - 4) * _G), ((N - 4, 3), I32)
    ar = Arena({}, outs, tail=4096)
    for i, seed in enumerate(ri.SEEDS):
        _call("tmf_rise_masks", ar.ptr(f"nodes{i}"), ar.ptr(f"shifts{i}"), *size, *cells, ri.P, seed, 0, N, _st())
    _call("tmf_rise_masks", ar.ptr("late_nodes"), ar.ptr("late_shifts"), *size, *cells, ri.P, ri.SEEDS[1], 4, N - 4, _st())
    got = ar.fetch()
    for i, seed in enumerate(ri.SEEDS):
        nodes, shifts = ri.masks_model(size, cells, ri.P, seed, 0, N)
        assert torch.equal(_bytes(got[f"nodes{i}"], (N,) + nn), nodes) and torch.equal(got[f"shifts{i}"], shifts), hex(seed)
    assert torch.equal(_bytes(got["late_nodes"], (N - 4,) + nn), _bytes(got["nodes1"], (N,) + nn)[4:])
    assert torch.equal(got["late_shifts"], got["shifts1"][4:])


@pytest.mark.parametrize("geom", ri.GEOMETRIES, ids=ri.geom_id)
def test_apply_kernel_equals_the_float32_twin(geom):
    """torch.equal with f + M * (vol - f) of the twin for K = 1, a chunk that crosses into the next sample and the short last
    chunk, with fill, with base, and with fill 0 equal to M * vol; the 16-byte path where D*H*W % 4 == 0 (the arena's slots are
    256-byte aligned), the scalar path otherwise and, on the % 4 == 0 cases, once more through an output that starts 4 bytes
    off."""
    from transmf_ad_amd import ops
    size, cells = geom
    vol, fill, base = ri.volumes(size)
    B, N, V = vol.shape[0], ri.MASKS, size[0] * size[1] * size[2]
    nodes, shifts = ri.masks_model(size, cells, ri.P, ri.SEEDS[1], 0, N)
    zero = torch.zeros(B)
    chunks = ri.chunkings(B, N)
    outs = {}
    for i, (_j0, K) in enumerate(chunks):
        for kind in ("fill", "base", "zero"):
            outs[f"{kind}{i}"] = ((K, 1) + size, F32)
    shifted = V % 4 == 0
    if shifted:
        outs["off"] = ((chunks[1][1] * V + 1,), F32)
    ar = Arena(dict(vol=vol, nodes=nodes, shifts=shifts, fill=fill, base=base, zero=zero), outs, tail=4096)
    geo = (B, *size, *cells, N)
    for i, (j0, K) in enumerate(chunks):
        _call("tmf_rise_apply", ar.ptr("vol"), ar.ptr("nodes"), ar.ptr("shifts"), ar.ptr("fill"), None, ar.ptr(f"fill{i}"), *geo, j0, K, _st())
        _call("tmf_rise_apply", ar.ptr("vol"), ar.ptr("nodes"), ar.ptr("shifts"), None, ar.ptr("base"), ar.ptr(f"base{i}"), *geo, j0, K, _st())
        _call("tmf_rise_apply", ar.ptr("vol"), ar.ptr("nodes"), ar.ptr("shifts"), ar.ptr("zero"), None, ar.ptr(f"zero{i}"), *geo, j0, K, _st())
    written = None
    if shifted:
        j0, K = chunks[1]
        _call("tmf_rise_apply", ar.ptr("vol"), ar.ptr("nodes"), ar.ptr("shifts"), ar.ptr("fill"), None, ar.ptr("off") + 4, *geo, j0, K, _st())
        written = {"off": torch.ones(K * V + 1, dtype=torch.bool)}
        written["off"][0] = False
    got = ar.fetch(written=written)
    M = ops.rise_mask_values(nodes, shifts, size, cells)
    for i, (j0, K) in enumerate(chunks):
        want = ops.rise_apply_torch(vol, nodes, shifts, fill, size, cells, j0, K)
        assert torch.equal(got[f"fill{i}"], want), (j0, K)
        assert torch.equal(got[f"base{i}"], ops.rise_apply_torch(vol, nodes, shifts, None, size, cells, j0, K, base=base)), (j0, K)
        for k in range(K):
            b, m = divmod(j0 + k, N)
            assert torch.equal(got[f"zero{i}"][k, 0], M[m] * vol[b, 0]), (j0, k)
        if shifted and i == 1:
            assert torch.equal(got["off"][1:].view(want.shape), want)


def _accumulate_case(size, cells, B, N, seed, device_ref=False):
    """-> (scores (B, N), nodes, shifts, scale = 1 / (N p), ref(scores, scale, m_first, m_step): the fp64 map on the host,
    computed on the device for the large geometry)."""
    from transmf_ad_amd import ops
    nodes, shifts = ri.masks_model(size, cells, ri.P, seed, 0, N)
    s = ri.scores_for(B, N)
    scale = 1.0 / (N * ri.P)
    dev = DEV if device_ref else "cpu"
    ref = lambda sc, sca, m_first, m_step: ops.rise_accumulate_torch(sc.double().to(dev), nodes.to(dev), shifts.to(dev), size, cells,
                                                                     sca, m_first, m_step, chunk=4).cpu()
    return s, nodes, shifts, scale, ref


@pytest.mark.parametrize("geom", ri.GEOMETRIES, ids=ri.geom_id)
def test_accumulate_kernel(geom):
    """Within the header's bound of the fp64 reference per sample row; the same bits in two calls; the same bits for sample 0
    alone and inside B = 3 and B = 9 (the group-of-8 seam is crossed: sample 8 is a group of its own); even plus odd halves
    within the bound of the whole; scores of ones within the bound of sum M."""
    size, cells = geom
    N = ri.MASKS
    s9, nodes, shifts, scale, ref = _accumulate_case(size, cells, 9, N, ri.SEEDS[2])
    ones = torch.ones((1, N))
    outs = {"b9": ((9,) + size, F32), "b9again": ((9,) + size, F32), "b3": ((3,) + size, F32), "b1": ((1,) + size, F32),
            "last": ((1,) + size, F32), "even": ((9,) + size, F32), "odd": ((9,) + size, F32), "cover": ((1,) + size, F32)}
    ar = Arena(dict(s9=s9, s3=s9[:3], s1=s9[:1], s8=s9[8:], ones=ones, nodes=nodes, shifts=shifts), outs, tail=4096)
    call = lambda sc, out, sca, B, m_first, m_step: _call("tmf_rise_accumulate", ar.ptr(sc), ar.ptr("nodes"), ar.ptr("shifts"),
                                                          ar.ptr(out), sca, B, *size, *cells, N, m_first, m_step, _st())
    call("s9", "b9", scale, 9, 0, 1)
    call("s9", "b9again", scale, 9, 0, 1)
    call("s3", "b3", scale, 3, 0, 1)
    call("s1", "b1", scale, 1, 0, 1)
    call("s8", "last", scale, 1, 0, 1)
    call("s9", "even", scale, 9, 0, 2)
    call("s9", "odd", scale, 9, 1, 2)
    call("ones", "cover", 1.0, 1, 0, 1)
    got = ar.fetch()
    assert torch.equal(got["b9"], got["b9again"])
    assert torch.equal(got["b3"], got["b9"][:3]) and torch.equal(got["b1"], got["b9"][:1]) and torch.equal(got["last"], got["b9"][8:])
    whole = ref(s9, scale, 0, 1)
    err, tol = ri.row_errors(got["b9"], whole), ri.map_tolerance(s9, scale, range(N))
    print(f"{ri.geom_id(geom)}: whole err / tol {(err / tol).max():.3f}")
    assert bool((err <= tol).all()), (err / tol).tolist()
    te, to = ri.map_tolerance(s9, scale, range(0, N, 2)), ri.map_tolerance(s9, scale, range(1, N, 2))
    ee, eo = ri.row_errors(got["even"], ref(s9, scale, 0, 2)), ri.row_errors(got["odd"], ref(s9, scale, 1, 2))
    eh = ri.row_errors(got["even"].double() + got["odd"].double(), whole)
    print(f"{ri.geom_id(geom)}: even err / tol {(ee / te).max():.3f} odd {(eo / to).max():.3f} even + odd {(eh / (te + to)).max():.3f}")
    assert bool((ee <= te).all()) and bool((eo <= to).all()) and bool((eh <= te + to).all())
    ec, tc = ri.row_errors(got["cover"], ref(ones, 1.0, 0, 1)), ri.map_tolerance(ones, 1.0, range(N))
    print(f"{ri.geom_id(geom)}: coverage err / tol {(ec / tc).max():.3f}")
    assert bool((ec <= tc).all()) and float(got["cover"].min()) >= 0 and float(got["cover"].max()) <= N * ri.MASK_MAX


def test_accumulate_kernel_strides_over_tiles():
    """More tiles than one grid-stride pass holds (RISE_ACC_MAX_TILES = 2048 of 1024 voxels) and a last tile that is not full:
    within the bound of fp64, every element written, two samples so that a group of 2 runs the run-time sample count."""
    size, cells = ri.STRIDING
    assert -(-size[0] * size[1] * size[2] // 1024) > 2048
    N = 3
    s, nodes, shifts, scale, ref = _accumulate_case(size, cells, 2, N, ri.SEEDS[0], device_ref=True)
    ar = Arena(dict(s=s, nodes=nodes, shifts=shifts), {"sal": ((2,) + size, F32)}, tail=4096)
    _call("tmf_rise_accumulate", ar.ptr("s"), ar.ptr("nodes"), ar.ptr("shifts"), ar.ptr("sal"), scale, 2, *size, *cells, N, 0, 1, _st())
    got = ar.fetch()
    err, tol = ri.row_errors(got["sal"], ref(s, scale, 0, 1)), ri.map_tolerance(s, scale, range(N))
    print(f"{ri.geom_id(ri.STRIDING)}: err / tol {(err / tol).max():.3f}")
    assert bool((err <= tol).all())


def test_entries_refuse_before_any_launch():
    """Bad arguments on real buffers full of a sentinel: a negative code, and every buffer unchanged."""
    from transmf_ad_amd import _lib
    lib = _lib.load()
    src = torch.full((2 * 512 + 64,), 7.0, device=DEV)
    dst = torch.full((8 * 512 + 64,), 7.0, device=DEV)
    nodes = torch.full((4 * 64 + 64,), 1, device=DEV, dtype=U8)
    shifts = torch.full((4 * 3 + 4,), 0, device=DEV, dtype=I32)
    p, q, n, s = src.data_ptr(), dst.data_ptr(), nodes.data_ptr(), shifts.data_ptr()
    geo = (8, 8, 8, 2, 2, 2)
    neg = lambda rc: rc < 0
    assert neg(lib.tmf_rise_masks(None, s, *geo, 0.5, 1, 0, 4, None)) and neg(lib.tmf_rise_masks(n, None, *geo, 0.5, 1, 0, 4, None))
    for p_ in (0.0, 1.0, float("nan")):
        assert neg(lib.tmf_rise_masks(n, s, *geo, p_, 1, 0, 4, None))
    for m0, N in ((0, 0), (-1, 4), (2 ** 31 - 2, 4)):
        assert neg(lib.tmf_rise_masks(n, s, *geo, 0.5, 1, m0, N, None))
    assert neg(lib.tmf_rise_masks(n, s + 2, *geo, 0.5, 1, 0, 4, None))
    apply = lambda vol=p, nd=n, sh=s, fill=p, base=None, out=q, B=2, g=geo, N=4, j0=0, K=1: \
        lib.tmf_rise_apply(vol, nd, sh, fill, base, out, B, *g, N, j0, K, None)
    acc = lambda sc=p, nd=n, sh=s, sal=q, B=2, g=geo, N=4, m_first=0, m_step=1: \
        lib.tmf_rise_accumulate(sc, nd, sh, sal, 1.0, B, *g, N, m_first, m_step, None)
    for kw in (dict(vol=None), dict(nd=None), dict(sh=None), dict(out=None), dict(fill=None), dict(B=0), dict(B=65537), dict(N=0),
               dict(g=(8, 0, 8, 2, 2, 2)), dict(g=(8, 8, 8, 2, 9, 2)), dict(g=(8, 8, 8, 0, 2, 2)), dict(g=(2048, 2048, 512, 2, 2, 2)),
               dict(j0=-1), dict(K=0), dict(j0=8), dict(j0=6, K=3), dict(K=65537), dict(vol=p + 2), dict(out=q + 1), dict(sh=s + 2),
               dict(fill=None, base=p + 2), dict(out=p), dict(out=p + 4 * 512), dict(vol=q + 4, out=q)):
        assert neg(apply(**kw)), kw
    for kw in (dict(sc=None), dict(nd=None), dict(sh=None), dict(sal=None), dict(B=0), dict(B=65537), dict(N=0), dict(g=(8, 8, 0, 2, 2, 2)),
               dict(g=(8, 8, 8, 2, 2, 9)), dict(m_step=0), dict(m_first=-1), dict(m_first=4), dict(sc=p + 2), dict(sal=q + 2), dict(sh=s + 1)):
        assert neg(acc(**kw)), kw
    assert b"tmf_rise_accumulate" in lib.tmf_last_error_string()
    torch.cuda.synchronize()
    assert bool((src == 7.0).all()) and bool((dst == 7.0).all()) and bool((nodes == 1).all()) and bool((shifts == 0).all())


# ---------------------------------------------------------------------------------------------------------------------
# the ops wrappers
# ---------------------------------------------------------------------------------------------------------------------

def _calls(monkeypatch, fn):
    """fn() -> (its result, the library entries it called in order)."""
    from transmf_ad_amd import _lib
    names, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    try:
        return fn(), names
    finally:
        monkeypatch.undo()


def test_ops_wrappers_route(monkeypatch):
    """Contiguous float32 HIP tensors take the kernels (one launch each), anything else the torch formulas: the same values;
    tmf_rise_geometry agrees with ops.rise_geometry."""
    from transmf_ad_amd import ops
    size, cells = ri.GEOMETRIES[4]
    vol, fill, base = ri.volumes(size)
    B, N = vol.shape[0], ri.MASKS
    want_n, want_s = ri.masks_model(size, cells, ri.P, ri.SEEDS[1], 0, N)
    (nodes, shifts), names = _calls(monkeypatch, lambda: ops.rise_masks(size, cells, ri.P, ri.SEEDS[1], 0, N, DEV))
    assert names == ["tmf_rise_masks"] and torch.equal(nodes.cpu(), want_n) and torch.equal(shifts.cpu(), want_s)
    tn, ts = ops.rise_masks_torch(size, cells, ri.P, ri.SEEDS[1], 0, N)                      # the library's, copied to the host
    assert tn.device.type == "cpu" and torch.equal(tn, want_n) and torch.equal(ts, want_s)
    hn, hs = ops._rise_masks_host(*ri.geometry(size, cells), ri.P, ri.SEEDS[1], 0, N)        # ... and the host restatement
    assert torch.equal(hn, want_n) and torch.equal(hs, want_s)
    v, f, b = vol.to(DEV), fill.to(DEV), base.to(DEV)
    assert ops.rise_ok(v, nodes, shifts, f) and not ops.rise_ok(vol, nodes) and not ops.rise_ok(v.double(), nodes)
    j0, K = ri.chunkings(B, N)[1]
    want = ops.rise_apply_torch(vol, want_n, want_s, fill, size, cells, j0, K)
    got, names = _calls(monkeypatch, lambda: ops.rise_apply(v, nodes, shifts, f, size, cells, j0, K))
    assert names == ["tmf_rise_apply"] and torch.equal(got.cpu(), want)
    buf = torch.empty((K + 3, 1) + size, device=DEV)
    got, names = _calls(monkeypatch, lambda: ops.rise_apply(v, nodes, shifts, None, size, cells, j0, K, base=b, out=buf[:K]))
    assert names == ["tmf_rise_apply"] and got.data_ptr() == buf.data_ptr()
    assert torch.equal(got.cpu(), ops.rise_apply_torch(vol, want_n, want_s, None, size, cells, j0, K, base=base))
    assert torch.equal(ops.rise_apply_torch(v, nodes, shifts, f, size, cells, j0, K).cpu(), want)         # the twin on the device
    wide = torch.zeros((B, 1) + size[:2] + (2 * size[2],), device=DEV)
    wide[..., ::2] = v
    got, names = _calls(monkeypatch, lambda: ops.rise_apply(wide[..., ::2], nodes, shifts, f, size, cells, j0, K))
    assert names == [] and torch.equal(got.cpu(), want)
    got, names = _calls(monkeypatch, lambda: ops.rise_apply(v.double(), nodes, shifts, f.double(), size, cells, j0, K))
    assert names == [] and got.dtype == F64
    s = ri.scores_for(B, N)
    ref = ops.rise_accumulate_torch(s.double(), want_n, want_s, size, cells, 0.25)
    tol = ri.map_tolerance(s, 0.25, range(N))
    got, names = _calls(monkeypatch, lambda: ops.rise_accumulate(s.to(DEV), nodes, shifts, size, cells, 0.25))
    assert names == ["tmf_rise_accumulate"] and bool((ri.row_errors(got.cpu(), ref) <= tol).all())
    got, names = _calls(monkeypatch, lambda: ops.rise_accumulate(s.to(DEV).double(), nodes, shifts, size, cells, 0.25))
    assert names == [] and float(ri.row_errors(got.cpu(), ref).max()) <= 1e-13


# ---------------------------------------------------------------------------------------------------------------------
# rise against the model's own forward
# ---------------------------------------------------------------------------------------------------------------------

def _score(logits, target, score="prob"):
    s = logits if score == "logit" else torch.softmax(logits, 1)
    return s.gather(1, target.view(-1, 1))[:, 0]


def _loop(net, vols, which, nodes, shifts, fills, size, cells, target, chunk, score="prob"):
    """The user's loop through the model's own forward: rise_apply_torch on the volumes `which`, in chunks of `chunk` jobs
    -> scores (B, N)."""
    from transmf_ad_amd import ops
    B, N = vols[0].shape[0], nodes.shape[0]
    outs = []
    with torch.no_grad():
        for j0 in range(0, B * N, chunk):
            K = min(chunk, B * N - j0)
            rows = torch.arange(j0, j0 + K, device=DEV) // N
            batch = [v.index_select(0, rows) for v in vols]
            for i in which:
                batch[i] = ops.rise_apply_torch(vols[i], nodes, shifts, fills[i], size, cells, j0, K)
            out = net(*batch)
            out = out[0] if isinstance(out, tuple) else out
            outs.append(_score(out, target.index_select(0, rows), score))
    return torch.cat(outs).view(B, N)


def _package_model(name):
    g = Golden(name)
    net = build(g, inject_masks=False).eval()
    mri, pet, _y = P.make_inputs(g.batch, g.size, seed=1234, kind="blobs")
    return net, [torch.from_numpy(mri).to(DEV), torch.from_numpy(pet).to(DEV)], tuple(g.size)


def _bits_follow_the_batch(enc, vol, N, chunk):
    """Whether the eval encoder gives some sample other bits in a chunk's batch than in the batch of the volumes themselves."""
    B = vol.shape[0]
    with torch.no_grad():
        base = enc(vol)
        for j0 in range(0, B * N, chunk):
            rows = torch.arange(j0, min(j0 + chunk, B * N), device=DEV) // N
            if not torch.equal(enc(vol.index_select(0, rows)), base.index_select(0, rows)):
                return True
    return False


@pytest.mark.parametrize("name", ("cnn_tiny", "ad_tiny"))
def test_rise_is_the_models_own_forward(name, monkeypatch):
    """reuse=False: Rise.scores equals, bit for bit, the model's own forward on batches the test builds with rise_apply_torch
    in the same chunks; one mask launch, one apply launch per chunk, one accumulate launch per map.  reuse=True: the same
    bits (or an encoder whose bits follow the batch size).  joint=True gives one map.  Parameters, buffers, .grads and
    torch's generator are unchanged."""
    import transmf_ad_amd as T
    from transmf_ad_amd import ops
    net, vols, size = _package_model(name)
    B, N, cells, chunk, seed = vols[0].shape[0], 6, 4, 5, ri.SEEDS[1]
    nchunks = -(-B * N // chunk)
    keep = {k: v.clone() for k, v in net.state_dict().items()}
    rng, rng_host = torch.cuda.get_rng_state(0), torch.get_rng_state()
    r, names = _calls(monkeypatch, lambda: T.rise(net, *vols, masks=N, cells=cells, seed=seed, chunk=chunk, reuse=False))
    assert names.count("tmf_rise_masks") == 1 and names.count("tmf_rise_apply") == 2 * nchunks
    assert names.count("tmf_rise_accumulate") == 2
    encoder_calls = names.count("tmf_snet_eval_fwd")             # the one-call encoders: 2 in the baseline, 2 per chunk and map
    nodes, shifts = ops.rise_masks(size, cells, 0.5, seed, 0, N, DEV)
    assert torch.equal(r.nodes, nodes) and torch.equal(r.shifts, shifts) and r.volumes == (0, 1) and r.cells == (4, 4, 4)
    target = r.logits.argmax(1)
    assert torch.equal(r.target, target) and torch.equal(r.base_score, _score(r.logits, target))
    zero = [torch.zeros(B, device=DEV)] * 2
    for i in (0, 1):
        want = _loop(net, vols, (i,), nodes, shifts, zero, size, cells, target, chunk)
        assert torch.equal(r.scores(i), want), i
        assert float((want - r.base_score.view(B, 1)).abs().max()) > 0
        ref = ops.rise_accumulate_torch(want.double(), nodes, shifts, size, cells, 1.0 / (N * 0.5))
        assert bool((ri.row_errors(r.map(i), ref) <= ri.map_tolerance(want, 1.0 / (N * 0.5), range(N))).all())
        assert torch.equal(r.mask(2), ops.rise_mask_values(nodes, shifts, size, cells)[2])
    re, names = _calls(monkeypatch, lambda: T.rise(net, *vols, masks=N, cells=cells, seed=seed, chunk=chunk, reuse=True))
    assert names.count("tmf_rise_apply") == 2 * nchunks
    assert encoder_calls in (0, 2 + 4 * nchunks) and names.count("tmf_snet_eval_fwd") == (2 + 2 * nchunks if encoder_calls else 0)
    for i in (0, 1):
        same = torch.equal(re.scores(i), r.scores(i)) and torch.equal(re.map(i), r.map(i))
        kept_enc, kept_vol = ((net.pet_cnn, vols[1]), (net.mri_cnn, vols[0]))[i]
        print(f"{name} volume {i}: max |scores(reuse=True) - scores(reuse=False)| = {float((re.scores(i) - r.scores(i)).abs().max()):.3e}")
        assert same or _bits_follow_the_batch(kept_enc, kept_vol, N, chunk), i
    joint, names = _calls(monkeypatch, lambda: T.rise(net, *vols, masks=N, cells=cells, seed=seed, chunk=chunk, joint=True))
    assert names.count("tmf_rise_accumulate") == 1 and torch.equal(joint.map(0), joint.map(1))
    assert torch.equal(joint.scores(), _loop(net, vols, (0, 1), nodes, shifts, zero, size, cells, target, chunk))
    with pytest.raises(ValueError, match="eval"):
        T.rise(net.train(), *vols, masks=N, cells=cells)
    net.eval()
    assert all(torch.equal(v, keep[k]) for k, v in net.state_dict().items()) and all(p.grad is None for p in net.parameters())
    assert torch.equal(torch.cuda.get_rng_state(0), rng) and torch.equal(torch.get_rng_state(), rng_host)


def test_rise_on_the_toy_model_against_rise_torch(monkeypatch):
    """The toy model of the host test on the device: scores bit for bit the model's own forward and equal to rise_torch's, the
    maps within the bound of each other's fp64; halves, coverage, baseline="blur", fill="mean" and a float64 module run; the
    planted cube is found."""
    import transmf_ad_amd as T
    from transmf_ad_amd import ops
    net = Cube().to(DEV).eval()
    size, cells, N, chunk = (16, 16, 16), 4, 64, 24
    x = cube_volumes(7).to(DEV)
    a, names = _calls(monkeypatch, lambda: T.rise(net, x, masks=N, cells=cells, seed=3, chunk=chunk, halves=True, score="logit", target=0))
    assert names.count("tmf_rise_apply") == -(-2 * N // chunk) and names.count("tmf_rise_accumulate") == 3
    b, names = _calls(monkeypatch, lambda: T.rise_torch(net, x, masks=N, cells=cells, seed=3, chunk=chunk, halves=True, score="logit", target=0))
    assert names == ["tmf_rise_masks"] and torch.equal(a.nodes, b.nodes) and torch.equal(a.shifts, b.shifts)
    want = _loop(net, [x], (0,), a.nodes, a.shifts, [torch.zeros(2, device=DEV)], size, (cells,) * 3, a.target, chunk, "logit")
    assert torch.equal(a.scores(), want) and torch.equal(b.scores(), want)
    scale = 1.0 / (N * 0.5)
    ref = ops.rise_accumulate_torch(want.double(), a.nodes, a.shifts, size, cells, scale)
    tol = ri.map_tolerance(want, scale, range(N))
    ea, eb = ri.row_errors(a.map(), ref), ri.row_errors(b.map(), ref)
    print(f"rise err / tol {(ea / tol.to(ea.device)).max():.3f}, rise_torch err / tol {(eb / tol.to(eb.device)).max():.3f}")
    assert bool((ea.cpu() <= tol.cpu()).all()) and bool((eb.cpu() <= tol.cpu()).all())
    for h, (m_first, n) in zip(a.halves(), ((0, 32), (1, 32))):
        href = ops.rise_accumulate_torch(want.double(), a.nodes, a.shifts, size, cells, 1.0 / (n * 0.5), m_first, 2)
        assert bool((ri.row_errors(h, href).cpu() <= ri.map_tolerance(want, 1.0 / (n * 0.5), range(m_first, N, 2)).cpu()).all())
    sh = a.split_half()
    assert tuple(sh.shape) == (2,) and bool((sh.abs() <= 1 + 1e-6).all())
    inside = net.inside(size).to(DEV)
    big = T.rise(net, cube_volumes(1).to(DEV), masks=256, cells=cells, seed=1, score="logit", target=0)       # the host test's case
    for s in big.map():
        assert float((s[inside].mean() - s[~inside].mean()) / s[~inside].std()) >= 1.0
    c, names = _calls(monkeypatch, lambda: T.rise(net, x, masks=N, cells=(2, 3, 4), seed=3, normalize="coverage", baseline="blur",
                                                  fill="mean", score="logit", target=0))
    assert names.count("tmf_rise_accumulate") == 2 and names.count("tmf_gaussian_smooth") >= 1
    ct = T.rise_torch(net, x, masks=N, cells=(2, 3, 4), seed=3, normalize="coverage", baseline="blur", score="logit", target=0)
    cover = ops.rise_accumulate_torch(torch.ones((1, N), device=DEV, dtype=F64), c.nodes, c.shifts, size, (2, 3, 4))[0]
    assert float(c.coverage.min()) >= 0 and float(c.coverage.max()) <= N * ri.MASK_MAX
    assert float((c.coverage.double() - cover).abs().max()) <= (N + 18) * 2.0 ** -24 * N
    # the two blurred bases differ by the smoothing kernel's own bound (about 70 * 2^-24 of the peak), the scores - means of the
    # volume - by no more, the maps - coverage-weighted means of the scores - by that plus the two accumulation bounds: 1e-5 of
    # the scores at most; held at 1e-4
    assert float((c.map() - ct.map()).abs().max()) <= 1e-4 * float(ct.scores().abs().max())
    d, names = _calls(monkeypatch, lambda: T.rise(Cube().double().to(DEV).eval(), x.double(), masks=8, cells=cells, seed=3))
    assert names == ["tmf_rise_masks"] and d.map().dtype == F64
