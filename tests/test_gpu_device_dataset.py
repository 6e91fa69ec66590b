"""Device-resident data set on the GPU: tmf_batch_augment bit for bit against the numpy restatement of
the reference's train transform (oracle/input_oracle.py), against the three single-stage kernels it fuses and against
DevicePrefetcher; the loader's epoch semantics, its one launch / no copy per batch, read-only stores, NIfTI construction
and a short training run fed by it.  Every comparison is exact."""
import numpy as np
import pytest
import torch

from oracle import input_oracle as IO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = np.nan


def _raw(B, shape, seed, lo=-50.0, hi=4000.0):
    rs = np.random.RandomState(seed)
    return (rs.rand(B, 1, *shape) * (hi - lo) + lo).astype(np.float32)


def _T():
    import transmf_ad_amd as T
    return T


def _P():
    from transmf_ad_amd import pipeline as P
    return P


def _batch(ds, idx, flips, angles, zooms):
    """One tmf_batch_augment launch with the decisions given."""
    P = _P()
    rec = P.pack_decisions(np.asarray(idx), np.asarray(flips, np.uint8), np.asarray(angles, float), np.asarray(zooms, float), ds.shape)
    out = ds.augment(torch.from_numpy(rec.view(np.uint8)).to(DEV), 0, len(idx))
    torch.cuda.synchronize()
    return out


# all eight flip / rotate / zoom combinations (sample b applies flip = b & 1, rotation = b & 2, zoom = b & 4); angles +-0.05
# and 0.0-but-applied; zooms 0.95, 0.9712 and exactly 1.0; subject 2 twice with different decisions; subject 3 is constant
IDX = [0, 1, 2, 3, 4, 5, 2, 3]
FLIPS = [0, 1, 0, 1, 0, 1, 0, 1]
ANGLES = [NAN, NAN, 0.05, -0.05, NAN, NAN, 0.0, -0.05]
ZOOMS = [NAN, NAN, NAN, NAN, 0.95, 0.9712, 1.0, 0.95]
CASES = {
    (7, 5, 3): (6, IDX, FLIPS, ANGLES, ZOOMS),
    (33, 20, 29): (6, IDX, FLIPS, ANGLES, ZOOMS),          # length-3 windows on the 33 axis (33 -> 31), odd pad difference on 20 -> 19
    (24, 20, 16): (6, IDX, FLIPS, ANGLES, ZOOMS),
    (91, 109, 91): (2, [1, 1], [1, 0], [0.05, -0.05], [0.95, NAN]),     # the ADNI shape: several blocks per plane, odd everything
}
_cache = {}


def _case(shape):
    """Raw volumes, the resident data set and ONE batch of a case; built once, shared by the tests, never modified."""
    if shape not in _cache:
        N, idx, flips, angles, zooms = CASES[shape]
        mri, pet = _raw(N, shape, 61), _raw(N, shape, 62, lo=0.0, hi=9.0)
        if N > 3:
            mri[3] = 12.5                                    # a constant volume -> zeros
        labels = (np.arange(N) * 3 + 1).astype(np.int64)
        ds = _T().DeviceDataset.from_arrays(mri, pet, labels, DEV)
        got = _batch(ds, idx, flips, angles, zooms)
        _cache[shape] = dict(mri=mri, pet=pet, labels=labels, ds=ds, idx=np.asarray(idx), flips=flips, angles=angles,
                             zooms=zooms, got={k: v.cpu().numpy() for k, v in got.items()})
    return _cache[shape]


@pytest.mark.parametrize("shape", list(CASES))
def test_batch_augment_equals_the_oracle_for_every_stage_combination(shape):
    c = _case(shape)
    assert {(bool(f), not np.isnan(a), not np.isnan(z)) for f, a, z in zip(FLIPS, ANGLES, ZOOMS)} == \
        {(f, a, z) for f in (False, True) for a in (False, True) for z in (False, True)}
    want_m, want_p = IO.train_transform(c["mri"][c["idx"]], c["pet"][c["idx"]], c["flips"], c["angles"], c["zooms"])
    assert c["got"]["MRI"].shape == want_m.shape and c["got"]["MRI"].dtype == np.float32
    assert np.array_equal(c["got"]["MRI"], want_m)           # bit for bit
    assert np.array_equal(c["got"]["PET"], want_p)
    assert c["got"]["label"].dtype == np.int64 and np.array_equal(c["got"]["label"], c["labels"][c["idx"]])
    if len(c["idx"]) == 8:
        assert not c["got"]["MRI"][3].any() and not c["got"]["MRI"][7].any()       # the constant subject
        assert not np.array_equal(c["got"]["MRI"][2], c["got"]["MRI"][6])          # one subject, two different samples


@pytest.mark.parametrize("shape", list(CASES))
def test_batch_augment_equals_the_three_kernels_in_sequence(shape):
    """scale_intensity_flip -> rotate_zoom on the gathered raw volumes: the kernels whose device functions the fused one
    shares.  No oracle involved."""
    T, c = _T(), _case(shape)
    fl = torch.tensor(c["flips"], dtype=torch.uint8, device=DEV)
    for key, raw in (("MRI", c["mri"]), ("PET", c["pet"])):
        x = T.scale_intensity_flip(torch.from_numpy(raw[c["idx"]]).to(DEV), fl)
        x = T.rotate_zoom(x, c["angles"], c["zooms"])
        torch.cuda.synchronize()
        assert np.array_equal(c["got"][key], x.cpu().numpy())
    # the stores themselves are ScaleIntensity of every subject
    assert np.array_equal(c["ds"].mri.cpu().numpy()[:, None],
                          T.scale_intensity_flip(torch.from_numpy(c["mri"]).to(DEV)).cpu().numpy())


def test_loader_equals_the_prefetcher_on_the_same_seed():
    T = _T()
    shape, N, B = (24, 20, 16), 8, 4
    mri, pet, labels = _raw(N, shape, 71), _raw(N, shape, 72), np.arange(N) % 2
    host = [dict(MRI=mri[s:s + B], PET=pet[s:s + B], label=labels[s:s + B]) for s in range(0, N, B)]
    kw = dict(seed=7, flip_prob=0.6, rotate_prob=0.6, zoom_prob=0.6)
    ds = T.DeviceDataset.from_arrays(mri, pet, labels, DEV)
    loader = ds.loader(batch_size=B, shuffle=False, **kw)
    assert len(loader) == 2
    n = applied = 0
    for a, b in zip(loader, T.DevicePrefetcher(host, device=DEV, **kw)):
        torch.cuda.synchronize()
        for k in ("MRI", "PET", "label"):
            assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
        for k in ("_flips", "_angles", "_zooms"):
            assert np.array_equal(a[k], b[k], equal_nan=True), k
        assert a["_index"].tolist() == list(range(n * B, n * B + B))
        applied += int(a["_flips"].sum()) + int((~np.isnan(a["_angles"])).sum()) + int((~np.isnan(a["_zooms"])).sum())
        n += 1
    assert n == 2 and applied > 0


def test_epoch_semantics():
    T = _T()
    shape, N = (7, 5, 3), 8
    mri, pet = _raw(N, shape, 81), _raw(N, shape, 82)
    ds = T.DeviceDataset.from_arrays(mri, pet, np.arange(N), DEV)            # label = subject number
    subset = [1, 2, 4, 5, 7]

    def epoch(loader):
        out = []
        for batch in loader:
            assert batch["MRI"].shape == (2, 1) + shape and batch["label"].tolist() == batch["_index"].tolist()
            out.append(batch)
        return out
    loader = ds.loader(indices=subset, batch_size=2, seed=3)
    assert len(loader) == 2
    e1, e2 = epoch(loader), epoch(loader)
    for e in (e1, e2):
        seen = np.concatenate([b["_index"] for b in e])
        assert len(seen) == 4 and len(set(seen.tolist())) == 4 and set(seen.tolist()) <= set(subset)
    assert np.concatenate([b["_index"] for b in e1]).tolist() != np.concatenate([b["_index"] for b in e2]).tolist()
    again = ds.loader(indices=subset, batch_size=2, seed=3)                   # the same seed: the same two epochs
    for e in (e1, e2):
        for a, b in zip(e, epoch(again)):
            assert a["_index"].tolist() == b["_index"].tolist() and torch.equal(a["MRI"], b["MRI"]) and torch.equal(a["PET"], b["PET"])
            assert np.array_equal(a["_angles"], b["_angles"], equal_nan=True)
    # evaluation: ScaleIntensity only, the order of `indices`, the short last batch kept
    val = ds.loader(indices=subset, batch_size=2, train=False)
    assert len(val) == 3
    batches = list(val)
    assert [b["_index"].tolist() for b in batches] == [[1, 2], [4, 5], [7]]
    for b in batches:
        assert not b["_flips"].any() and np.isnan(b["_angles"]).all() and np.isnan(b["_zooms"]).all()
        wm, wp = IO.train_transform(mri[b["_index"]], pet[b["_index"]], b["_flips"])
        assert np.array_equal(b["MRI"].cpu().numpy(), wm) and np.array_equal(b["PET"].cpu().numpy(), wp)
    with pytest.raises(T.TmfError, match="outside"):
        ds.loader(indices=[0, N], batch_size=2)
    assert ds.loader(batch_size=3, drop_last=False).__len__() == 3 and ds.loader(batch_size=3).__len__() == 2


def _device_events(fn):
    """(kernel names, memcpy names) of the device activity of fn() (torch.profiler), after a warm-up call."""
    from torch.profiler import ProfilerActivity, profile
    from torch.autograd import DeviceType
    fn()                                         # warm-up: lazy module loading, allocator
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == DeviceType.CUDA]
    copies = [n for n in names if n.lower().startswith("memcpy")]
    kernels = [n for n in names if not n.lower().startswith(("memcpy", "memset"))]
    return kernels, copies


def test_one_launch_per_batch_and_one_copy_per_epoch():
    c = _case((24, 20, 16))
    loader = c["ds"].loader(batch_size=2, seed=1, flip_prob=0.6, rotate_prob=0.6, zoom_prob=0.6)
    assert len(loader) == 3
    state = {}

    def start():                                  # a new epoch: the plan goes up; the first batch is one launch as well
        state["it"] = iter(loader)
        state["b"] = next(state["it"])
    kernels, copies = _device_events(start)
    print("epoch start:", kernels, copies)
    assert len(copies) == 1 and "htod" in copies[0].lower().replace(" ", ""), copies
    assert len(kernels) == 1 and "batch_augment_kernel" in kernels[0], kernels

    def mid():                                    # a mid-epoch next()
        state["b"] = next(state["it"])
    start()
    torch.cuda.synchronize()
    from torch.profiler import ProfilerActivity, profile
    from torch.autograd import DeviceType
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        mid()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == DeviceType.CUDA]
    print("mid-epoch next():", names)
    assert len(names) == 1 and "batch_augment_kernel" in names[0], names        # one kernel; no memcpy, no memset


def test_stores_are_read_only_and_batches_do_not_alias_them():
    c = _case((24, 20, 16))
    ds = c["ds"]
    before = (ds.mri.clone(), ds.pet.clone(), ds.labels.clone())
    spans = [(t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()) for t in (ds.mri, ds.pet, ds.labels)]
    kept = []
    for batch in ds.loader(batch_size=2, seed=5, flip_prob=0.6, rotate_prob=0.6, zoom_prob=0.6):
        kept.append(batch)                        # held, so that no two batches share memory either
        for k in ("MRI", "PET", "label"):
            lo = batch[k].data_ptr()
            hi = lo + batch[k].numel() * batch[k].element_size()
            assert all(hi <= a or lo >= b for a, b in spans), k
    torch.cuda.synchronize()
    assert len(kept) == 3
    assert torch.equal(ds.mri, before[0]) and torch.equal(ds.pet, before[1]) and torch.equal(ds.labels, before[2])


def test_from_nifti_equals_from_arrays(tmp_path):
    T = _T()
    rs = np.random.RandomState(9)
    vols = [(rs.rand(16, 20, 12) * 900).astype(np.float32) for _ in range(8)]
    mp, pp = [], []
    for k in range(4):
        T.write_nifti(str(tmp_path / f"m{k}.nii.gz"), vols[2 * k])
        T.write_nifti(str(tmp_path / f"p{k}.nii.gz"), vols[2 * k + 1])
        mp.append(str(tmp_path / f"m{k}.nii.gz")); pp.append(str(tmp_path / f"p{k}.nii.gz"))
    labels = [0, 1, 1, 0]
    a = T.DeviceDataset.from_nifti(mp, pp, labels, DEV)
    b = T.DeviceDataset.from_arrays(np.stack(vols[0::2])[:, None], np.stack(vols[1::2]), labels, DEV)   # (N, 1, ...) and (N, ...)
    assert a.shape == b.shape == (16, 20, 12) and len(a) == 4
    assert torch.equal(a.mri, b.mri) and torch.equal(a.pet, b.pet) and torch.equal(a.labels, b.labels)
    assert np.array_equal(a.mri.cpu().numpy(), np.stack([IO.scale_intensity(v) for v in vols[0::2]]))
    T.write_nifti(str(tmp_path / "odd.nii.gz"), vols[0][:, :19])
    with pytest.raises(T.TmfError, match="odd.nii.gz"):
        T.DeviceDataset.from_nifti(mp, pp[:2] + [str(tmp_path / "odd.nii.gz")] + pp[3:], labels, DEV)
    with pytest.raises(T.TmfError, match=r"MRI\[1\]"):
        T.DeviceDataset.from_arrays([vols[0], vols[0][:, :19], vols[2]], [vols[1], vols[3], vols[5]], [0, 1, 0], DEV)


def test_a_data_set_that_does_not_fit_is_refused_with_both_numbers():
    T = _T()
    v = np.zeros((64, 64, 64), np.float32)

    class Many:                                   # 4 M subjects of 1 MiB each and modality: far beyond any device
        def __len__(self):
            return 1 << 22

        def __getitem__(self, i):
            return v
    free = torch.cuda.mem_get_info(torch.device(DEV))[0]
    with pytest.raises(T.TmfError, match=r"need \d+ bytes.* \d+ bytes are free") as e:
        T.DeviceDataset.from_arrays(Many(), Many(), np.zeros(1 << 22, np.int64), DEV)
    need = 2 * (1 << 22) * v.size * 4
    assert any(int(w) >= need for w in str(e.value).replace(",", " ").split() if w.isdigit())
    assert torch.cuda.mem_get_info(torch.device(DEV))[0] >= free - (64 << 20)       # nothing of it was allocated


def test_two_training_steps_fed_by_the_loader():
    """model_ad on 32^3 batches out of a resident data set: finite losses, parameters move, and the batches are what the
    encoder's one-call path wants (contiguous float32 on the device, no gradient)."""
    T = _T()
    from transmf_ad_amd import ops
    from transmf_ad_amd.optim import Adam
    shape, N, B = (32, 32, 32), 6, 2
    ds = T.DeviceDataset.from_arrays(_raw(N, shape, 91), _raw(N, shape, 92), np.arange(N) % 2, DEV)
    torch.manual_seed(0)
    net = T.model_ad(dim=32, depth=1, heads=4, dim_head=8, mlp_dim=128, dropout=0.0).to(DEV).train()
    opt = Adam(net.parameters(), lr=1e-4)
    crit = torch.nn.CrossEntropyLoss()
    enc = net.mri_cnn
    blocks = [(getattr(enc, n)[i], getattr(enc, n)[i + 1], getattr(enc, n)[i + 2]) for n, i, _ in enc._PLAN]
    w0 = blocks[0][0].weight.detach().clone()
    losses = []
    for step, batch in enumerate(ds.loader(batch_size=B, seed=2)):
        if step == 2:
            break
        mri, pet, label = batch["MRI"], batch["PET"], batch["label"]
        for x in (mri, pet):
            assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and not x.requires_grad
            assert x.shape == (B, 1) + shape
        assert enc._one_call_ok(mri, blocks, prec=ops.resolve_precision(enc.tmf_precision))
        opt.zero_grad()
        lo, dm, dp = net(mri, pet)
        loss = (crit(dm, torch.ones_like(label)) + crit(dp, torch.zeros_like(label))) / 2 + crit(lo, label)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert len(losses) == 2 and all(np.isfinite(losses)), losses
    assert not torch.equal(blocks[0][0].weight.detach(), w0)
