"""Input pipeline ahead of the hot path, on the device.

The reference feeds `train_step` from a MONAI `DataLoader(num_workers=0)` (datasets/__init__.py:56): NIfTI load,
`ScaleIntensityd`, `RandFlipd(prob=0.3, spatial_axis=0)`, `RandRotated(prob=0.3, range_x=0.05)`,
`RandZoomd(prob=0.3, min_zoom=0.95, max_zoom=1)` on the host (datasets/ADNI.py:59-70), then `batch['MRI'].to(device)`
inside the step (kfold_train_adversarial.py:106-108).  Here the RAW volumes go to the device on a copy stream (the copy
of batch i + 1 overlaps the step of batch i) and all four transforms run there as HIP kernels
(csrc/input_pipeline.hip, bit-identical to MONAI's published algorithms as restated in oracle/input_oracle.py).  The
random DECISIONS (flip?, rotate? and the angle, zoom? and the factor) are drawn on the host with numpy, one set per
subject shared by MRI and PET as MONAI's dictionary transforms do (MONAI draws them from its own RandomState; only the
probabilities and ranges are part of the reference's configuration).  `nifti.read_nifti` / `nifti_batches` read
`.nii` / `.nii.gz` volumes in the prefetcher's worker thread (datasets/ADNI.py:62 LoadImaged).

`DeviceDataset` keeps a whole data set on the device instead (the reference's CacheDataset, datasets/__init__.py:12-29,
with HBM as the cache): loading, ScaleIntensity and the host-to-device copy happen once per run, and every training batch
of a `DeviceDataset.loader` is ONE `tmf_batch_augment` launch that gathers, flips, rotates and zooms out of the resident
stores — no copy, no side stream, no worker thread.
"""
from __future__ import annotations

import math
from typing import Iterable, Iterator, Optional, Sequence

import numpy as np
import torch

from . import _lib


def draw_decisions(rs: np.random.RandomState, B: int, flip_prob: float, rotate_prob: float, rotate_range: float,
                   zoom_prob: float, zoom_range) -> tuple:
    """The random decisions of one batch of B subjects -> (flips uint8 (B,), angles float64 (B,), zooms float64 (B,); NaN =
    not applied).  One set per subject, shared by MRI and PET (MONAI dictionary transforms); per transform the "apply?" draw
    first, then its parameters (RandRotated draws x, y, z — y and z from (0, 0); RandZoomd one factor).  The ONE place
    these are drawn: DevicePrefetcher and DeviceDataset.loader consume a RandomState identically."""
    flips = (rs.random_sample(B) < flip_prob).astype(np.uint8)
    angles = np.full(B, np.nan)
    zooms = np.full(B, np.nan)
    if rotate_prob > 0:
        for b in range(B):
            if rs.random_sample() < rotate_prob:
                angles[b] = rs.uniform(-rotate_range, rotate_range)
                rs.uniform(0.0, 0.0); rs.uniform(0.0, 0.0)
    if zoom_prob > 0:
        for b in range(B):
            if rs.random_sample() < zoom_prob:
                zooms[b] = rs.uniform(*zoom_range)
    return flips, angles, zooms


def rotation_cos_sin(angle: float) -> tuple:
    """(cos, sin) of a rotation angle as the kernels take them: evaluated in double, rounded to fp32 once."""
    return np.float32(math.cos(angle)), np.float32(math.sin(angle))


def zoom_out_size(shape, zoom: float) -> list:
    """Zoom's output size floor(S z) per axis of `shape`; only 0 < zoom <= 1 is provided (RandZoomd(0.95, 1))."""
    o = [int(math.floor(float(n) * zoom)) for n in shape]
    if min(o) < 1 or any(a > n for a, n in zip(o, shape)):
        raise _lib.TmfError(f"zoom factor {zoom}: only 0 < zoom <= 1 is provided (RandZoomd(0.95, 1))")
    return o


def scale_intensity_flip(vol: torch.Tensor, flips: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                         stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
    """ScaleIntensity (per volume min-max to [0, 1]) and Flip(spatial_axis=0) of a device batch (B, 1, D, H, W) / (B, D, H, W).
    flips: uint8 device tensor (B,), non-zero = reverse the first spatial axis of that volume."""
    if not vol.is_cuda or vol.dtype != torch.float32:
        raise _lib.TmfError("scale_intensity_flip needs a float32 tensor on the HIP device (there is no CPU fallback)")
    v = vol.contiguous()
    B = v.shape[0]
    D, H, W = v.shape[-3:]
    if v.numel() != B * D * H * W:
        raise _lib.TmfError(f"expected (B, 1, D, H, W) or (B, D, H, W), got {tuple(vol.shape)}")
    if flips is not None and not (flips.is_cuda and flips.dtype == torch.uint8 and flips.numel() == B):
        raise _lib.TmfError("flips must be a uint8 device tensor of B elements")
    with torch.cuda.device(v.device), (torch.cuda.stream(stream) if stream is not None else _Null()):
        # allocations and launches under the SAME current stream (the caching allocator ties a block to its stream)
        out = torch.empty_like(v) if out is None else out
        s = torch.cuda.current_stream(v.device).cuda_stream
        nws = _lib.query("tmf_scale_intensity_workspace_bytes", B)
        ws = torch.empty(nws // 4 + 2 * B, device=v.device, dtype=torch.float32)
        minmax = ws[nws // 4:]
        _lib.call("tmf_volume_minmax", v.data_ptr(), minmax.data_ptr(), ws.data_ptr(), nws, B, D * H * W, s)
        _lib.call("tmf_scale_flip", v.data_ptr(), out.data_ptr(), minmax.data_ptr(),
                  None if flips is None else flips.data_ptr(), B, D, H, W, s)
    return out


def rotate_zoom(vol: torch.Tensor, angles=None, zooms=None, stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
    """RandRotated / RandZoomd (datasets/ADNI.py:67-68) of a device batch (B, 1, D, H, W) with the decisions given: angles[b]
    (radians about the first spatial axis; NaN / None = no rotation), zooms[b] (factor in (0, 1]; NaN / None = no zoom).
    Bit-identical to oracle/input_oracle.py rotate_x / zoom_area."""
    if not vol.is_cuda or vol.dtype != torch.float32:
        raise _lib.TmfError("rotate_zoom needs a float32 tensor on the HIP device (there is no CPU fallback)")
    v = vol.contiguous()
    B = v.shape[0]
    D, H, W = v.shape[-3:]
    if v.numel() != B * D * H * W:
        raise _lib.TmfError(f"expected (B, 1, D, H, W) or (B, D, H, W), got {tuple(vol.shape)}")
    def decisions(vals):
        if vals is None:
            return [None] * B
        if len(vals) != B:
            raise _lib.TmfError(f"expected {B} per-volume decisions, got {len(vals)}")
        return [None if (x is None or math.isnan(float(x))) else float(x) for x in vals]
    ang, zs = decisions(angles), decisions(zooms)
    with torch.cuda.device(v.device), (torch.cuda.stream(stream) if stream is not None else _Null()):
        s = torch.cuda.current_stream(v.device).cuda_stream
        if any(a is not None for a in ang):
            cs = np.zeros((B, 2), np.float32)
            flag = np.zeros(B, np.uint8)
            for b_, a in enumerate(ang):
                if a is not None:
                    cs[b_] = rotation_cos_sin(a)
                    flag[b_] = 1
            out = torch.empty_like(v)
            cs_d, flag_d = torch.from_numpy(cs).to(v.device), torch.from_numpy(flag).to(v.device)     # held until the call returns
            _lib.call("tmf_rotate_x", v.data_ptr(), out.data_ptr(), cs_d.data_ptr(), flag_d.data_ptr(), B, D, H, W, s)
            v = out
        if any(z is not None for z in zs):
            sz = np.zeros((B, 3), np.int32)
            flag = np.zeros(B, np.uint8)
            for b_, z in enumerate(zs):
                if z is not None:
                    sz[b_] = zoom_out_size((D, H, W), z)
                    flag[b_] = 1
            out = torch.empty_like(v)
            sz_d, flag_d = torch.from_numpy(sz).to(v.device), torch.from_numpy(flag).to(v.device)
            _lib.call("tmf_zoom_area", v.data_ptr(), out.data_ptr(), sz_d.data_ptr(), flag_d.data_ptr(), B, D, H, W, s)
            v = out
    return v.view(vol.shape)


class _Null:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


class DevicePrefetcher:
    """Iterate device batches {'MRI', 'PET', 'label'} from an iterable of HOST batches with the same keys (numpy arrays
    or CPU tensors; MRI / PET raw float32 volumes (B, 1, D, H, W)).  Batch i + 1 is staged into pinned memory and copied
    on a side stream while the caller trains on batch i; ScaleIntensity + flip run on that side stream too."""

    def __init__(self, batches: Iterable, device="cuda", flip_prob: float = 0.3, seed: Optional[int] = None,
                 train: bool = True, rotate_prob: float = 0.3, rotate_range: float = 0.05, zoom_prob: float = 0.3,
                 zoom_range=(0.95, 1.0), pinned_staging: bool = False):
        """train=True applies the reference's whole augmentation set with its probabilities and ranges
        (datasets/ADNI.py:66-68); set a probability to 0 to leave a transform out.  train=False: ScaleIntensity only
        (the reference's test_transform)."""
        self.batches = batches
        self.device = torch.device(device)
        self.flip_prob = flip_prob if train else 0.0
        self.rotate_prob = rotate_prob if train else 0.0
        self.rotate_range = float(rotate_range)
        self.zoom_prob = zoom_prob if train else 0.0
        self.zoom_range = (float(zoom_range[0]), float(zoom_range[1]))
        self.rs = np.random.RandomState(seed)
        self.copy_stream = torch.cuda.Stream(device=self.device)
        self._pinned = [dict(), dict()]          # two staging sets, reused while shapes stay the same
        # pinned_staging=False (default): the worker thread copies straight from the loader's pageable arrays with a
        # blocking .to(device) on the copy stream — the runtime stages through its own pinned pool at the full link rate
        # (50 GB/s measured here), and only the WORKER blocks.  Re-filling our own pinned set every batch measured 15 ms
        # per 28 MB on this box (tools/prefetch_probe.py), slower than the copy it was meant to speed up.
        self.pinned_staging = pinned_staging

    def _stage(self, slot, key, arr):
        t = torch.as_tensor(arr)
        if not self.pinned_staging:
            return t
        buf = self._pinned[slot].get(key)
        if buf is None or buf.shape != t.shape or buf.dtype != t.dtype:
            buf = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
            self._pinned[slot][key] = buf
        buf.copy_(t)
        return buf

    def _launch(self, slot, host_batch):
        B = len(host_batch["label"])
        flips, angles, zooms = draw_decisions(self.rs, B, self.flip_prob, self.rotate_prob, self.rotate_range,
                                              self.zoom_prob, self.zoom_range)
        with torch.cuda.stream(self.copy_stream):
            out = {}
            nb = self.pinned_staging
            fl = self._stage(slot, "_flips", flips).to(self.device, non_blocking=nb)
            for key in ("MRI", "PET"):
                raw = self._stage(slot, key, host_batch[key]).to(self.device, non_blocking=nb)
                x = scale_intensity_flip(raw, fl if self.flip_prob > 0 else None, stream=self.copy_stream)
                if not (np.isnan(angles).all() and np.isnan(zooms).all()):
                    x = rotate_zoom(x, angles, zooms, stream=self.copy_stream)
                out[key] = x
            out["label"] = self._stage(slot, "label", np.asarray(host_batch["label"], dtype=np.int64)).to(
                self.device, non_blocking=nb)
            out["_flips"], out["_angles"], out["_zooms"] = flips, angles, zooms
            ev = torch.cuda.Event()
            ev.record(self.copy_stream)
        return out, ev

    def __iter__(self) -> Iterator[dict]:
        """A worker thread stages batch i + 1 (pageable -> pinned memcpy, H2D and the two kernels on the copy stream) while
        the caller trains on batch i: the main thread only waits on an event.  (Staging from the training thread itself
        serialises a 57 MB host memcpy per step with the kernel launches: 36 ms per step instead of 17.)"""
        import queue
        import threading
        q: "queue.Queue" = queue.Queue(maxsize=1)          # one batch ready + one being staged = the two pinned sets
        stop = threading.Event()
        dev = self.device

        def worker():
            try:
                torch.cuda.set_device(dev)
                events = [None, None]
                slot = 0
                for host_batch in self.batches:
                    if stop.is_set():
                        break
                    if events[slot] is not None:
                        events[slot].synchronize()          # the copies out of this pinned set have completed
                    out, ev = self._launch(slot, host_batch)
                    events[slot] = ev
                    slot ^= 1
                    while not stop.is_set():
                        try:
                            q.put((out, ev), timeout=0.1)
                            break
                        except queue.Full:
                            continue
                q.put(None)
            except BaseException as e:                       # surface worker failures in the training thread
                q.put(e)

        # The training thread is busy issuing launches for most of a step and only hands the GIL over every
        # sys.getswitchinterval() = 5 ms; the worker needs it ~30 times per batch (between its GIL-free copies and
        # launches), so with the default interval a 1 ms staging job stretches to tens of ms and the step waits for it
        # (measured: 36 ms per step instead of 17).  A 100 us interval while the prefetcher runs costs the trainer nothing
        # measurable and lets the worker through.
        import sys
        old_interval = sys.getswitchinterval()
        sys.setswitchinterval(1e-4)
        th = threading.Thread(target=worker, name="tmf-prefetch", daemon=True)
        th.start()
        try:
            while True:
                item = q.get()
                if item is None:
                    return
                if isinstance(item, BaseException):
                    raise item
                out, ev = item
                cur = torch.cuda.current_stream(self.device)
                cur.wait_event(ev)
                for k in ("MRI", "PET", "label"):
                    out[k].record_stream(cur)
                yield out
        finally:
            sys.setswitchinterval(old_interval)
            stop.set()
            while th.is_alive():
                try:
                    q.get_nowait()
                except queue.Empty:
                    pass
                th.join(timeout=0.05)


# ---------------------------------------------------------------------------------------------------------------------
# Device-resident data set: every subject in HBM for the run, one launch per training batch
# ---------------------------------------------------------------------------------------------------------------------

# tmf_augment_decision (include/tmf_hip.h), field by field
DECISION_DTYPE = np.dtype([("index", "<i4"), ("flip", "<i4"), ("do_rot", "<i4"), ("cos_a", "<f4"), ("sin_a", "<f4"),
                           ("od", "<i4"), ("oh", "<i4"), ("ow", "<i4")])
assert DECISION_DTYPE.itemsize == 32


def validate_indices(indices, n: int) -> np.ndarray:
    """A subset of the subjects [0, n) (a fold, or one side of its train / val split) -> int64 array; None = all of them.
    Raises on anything else, on the host, before a record is packed."""
    if indices is None:
        return np.arange(n, dtype=np.int64)
    idx = np.asarray(indices)
    if idx.ndim != 1 or idx.size == 0:
        raise _lib.TmfError(f"indices must be a non-empty 1-D sequence of subject numbers, got shape {idx.shape}")
    if idx.dtype == np.bool_ or not np.issubdtype(idx.dtype, np.integer):
        raise _lib.TmfError(f"indices must be integers, got dtype {idx.dtype}")
    bad = np.flatnonzero((idx < 0) | (idx >= n))
    if bad.size:
        raise _lib.TmfError(f"indices[{int(bad[0])}] = {int(idx[bad[0]])} is outside [0, {n})")
    return idx.astype(np.int64)


def pack_decisions(index, flips, angles, zooms, shape) -> np.ndarray:
    """Decision records (DECISION_DTYPE) of the samples whose subject, flip, angle and zoom factor are given (NaN = not
    applied), for volumes of `shape` = (D, H, W)."""
    rec = np.zeros(len(index), DECISION_DTYPE)
    rec["index"] = index
    rec["flip"] = flips
    for b, (a, z) in enumerate(zip(angles, zooms)):
        if not math.isnan(a):
            rec["do_rot"][b] = 1
            rec["cos_a"][b], rec["sin_a"][b] = rotation_cos_sin(float(a))
        if not math.isnan(z):
            rec["od"][b], rec["oh"][b], rec["ow"][b] = zoom_out_size(shape, float(z))
    return rec


def epoch_plan(rs: np.random.RandomState, indices: np.ndarray, batch_size: int, shuffle: bool, drop_last: bool, shape,
               flip_prob: float, rotate_prob: float, rotate_range: float, zoom_prob: float, zoom_range) -> tuple:
    """One epoch over `indices`, drawn on the host in one go -> (records, batches): `records` holds the decision record of
    every sample of the epoch in order (one upload), `batches` one dict per batch with its slice `start` / `stop` of the
    records and the decisions as DevicePrefetcher reports them (`_index`, `_flips`, `_angles`, `_zooms`).  Draw order: the
    permutation first (when shuffling), then draw_decisions batch by batch."""
    order = indices[rs.permutation(len(indices))] if shuffle else indices
    stop = len(order) - len(order) % batch_size if drop_last else len(order)
    recs, batches = [], []
    for s in range(0, stop, batch_size):
        sel = order[s:min(s + batch_size, stop)]
        flips, angles, zooms = draw_decisions(rs, len(sel), flip_prob, rotate_prob, rotate_range, zoom_prob, zoom_range)
        recs.append(pack_decisions(sel, flips, angles, zooms, shape))
        batches.append(dict(start=s, stop=s + len(sel), _index=sel, _flips=flips, _angles=angles, _zooms=zooms))
    return (np.concatenate(recs) if recs else np.zeros(0, DECISION_DTYPE)), batches


class DeviceLoader:
    """Re-iterable batches out of a DeviceDataset (DeviceDataset.loader): every __iter__ draws a fresh epoch."""

    def __init__(self, dataset: "DeviceDataset", indices, batch_size: int, train: bool, shuffle, drop_last, seed,
                 flip_prob, rotate_prob, rotate_range, zoom_prob, zoom_range):
        self.dataset = dataset
        self.indices = validate_indices(indices, dataset.n)
        self.batch_size = int(batch_size)
        if not 1 <= self.batch_size <= 32767:
            raise _lib.TmfError(f"batch_size {batch_size} is outside [1, 32767] (one launch: 2 * batch_size grid planes)")
        self.shuffle = train if shuffle is None else bool(shuffle)
        self.drop_last = train if drop_last is None else bool(drop_last)
        self.flip_prob = flip_prob if train else 0.0
        self.rotate_prob = rotate_prob if train else 0.0
        self.rotate_range = float(rotate_range)
        self.zoom_prob = zoom_prob if train else 0.0
        self.zoom_range = (float(zoom_range[0]), float(zoom_range[1]))
        self.rs = np.random.RandomState(seed)

    def __len__(self) -> int:
        n = len(self.indices)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def __iter__(self) -> Iterator[dict]:
        ds = self.dataset
        records, batches = epoch_plan(self.rs, self.indices, self.batch_size, self.shuffle, self.drop_last, ds.shape,
                                      self.flip_prob, self.rotate_prob, self.rotate_range, self.zoom_prob, self.zoom_range)
        if not batches:
            return
        with torch.cuda.device(ds.device):
            plan = torch.from_numpy(records.view(np.uint8)).to(ds.device)              # the epoch's ONE host-to-device copy
        for b in batches:
            out = ds.augment(plan, b["start"], b["stop"] - b["start"])
            out.update(_index=b["_index"], _flips=b["_flips"], _angles=b["_angles"], _zooms=b["_zooms"])
            yield out


class DeviceDataset:
    """Every subject of a data set on the device for the whole run: `mri` / `pet` (N, D, H, W) float32 AFTER ScaleIntensity
    (the deterministic part of the reference's transform, cached as its CacheDataset does: datasets/__init__.py:12-29) and
    `labels` (N,) int64.  One data set serves any number of loaders — the folds of a k-fold run
    (kfold_train_adversarial.py:60-66) are `loader(indices=...)` over the same resident stores."""

    CHUNK = 4            # subjects per upload: bounds the raw staging copy next to the stores

    def __init__(self, mri: torch.Tensor, pet: torch.Tensor, labels: torch.Tensor):
        self.mri, self.pet, self.labels = mri, pet, labels
        self.n = int(mri.shape[0])
        self.shape = tuple(int(s) for s in mri.shape[1:])
        self.device = mri.device

    def __len__(self) -> int:
        return self.n

    def augment(self, plan: torch.Tensor, start: int, count: int) -> dict:
        """One batch in ONE launch on the current stream: `plan` is a device tensor of decision records (DECISION_DTYPE, as
        bytes: pack_decisions / epoch_plan), of which records [start, start + count) make this batch.  The subjects the
        records name must lie in [0, N) (DeviceDataset.loader validates them on the host).  -> {'MRI', 'PET': (count, 1, D,
        H, W) float32, 'label': (count,) int64}, freshly allocated."""
        item = DECISION_DTYPE.itemsize
        if not (plan.is_cuda and plan.device == self.device and plan.dtype == torch.uint8 and plan.is_contiguous()):
            raise _lib.TmfError("plan must be a contiguous uint8 tensor of decision records on the data set's device")
        if not (0 <= start and 1 <= count and (start + count) * item <= plan.numel()):
            raise _lib.TmfError(f"records [{start}, {start + count}) are outside a plan of {plan.numel() // item} records")
        D, H, W = self.shape
        with torch.cuda.device(self.device):
            cur = torch.cuda.current_stream(self.device)
            plan.record_stream(cur)                      # (a no-op on the stream the plan was uploaded on)
            mri = torch.empty((count, 1, D, H, W), device=self.device, dtype=torch.float32)
            pet = torch.empty_like(mri)
            label = torch.empty(count, device=self.device, dtype=torch.int64)
            _lib.call("tmf_batch_augment", self.mri.data_ptr(), self.pet.data_ptr(), self.labels.data_ptr(),
                      plan.data_ptr() + start * item, mri.data_ptr(), pet.data_ptr(), label.data_ptr(),
                      self.n, count, D, H, W, cur.cuda_stream)
        return {"MRI": mri, "PET": pet, "label": label}

    @classmethod
    def _build(cls, n: int, volume, what, labels, device) -> "DeviceDataset":
        """volume(key, i) -> subject i's host volume of modality key ('MRI' | 'PET'), read ONCE; what(key, i) names it."""
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.TmfError("DeviceDataset needs a HIP device (there is no CPU fallback)")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        lab = np.asarray(labels)
        if n < 1 or lab.shape != (n,) or not np.issubdtype(lab.dtype, np.integer):
            raise _lib.TmfError(f"need N >= 1 subjects and N integer labels, got N = {n} and labels of shape {lab.shape} {lab.dtype}")

        def host_volume(key, i):
            v = torch.as_tensor(volume(key, i))
            if v.dim() == 4 and v.shape[0] == 1:
                v = v[0]
            if v.dim() != 3 or v.dtype != torch.float32 or v.is_cuda:
                raise _lib.TmfError(f"{what(key, i)}: expected a float32 host volume (D, H, W) or (1, D, H, W), "
                                    f"got {tuple(v.shape)} {v.dtype}")
            return v

        stores, shape = {}, None
        for c0 in range(0, n, cls.CHUNK):
            sel = range(c0, min(c0 + cls.CHUNK, n))
            for key in ("MRI", "PET"):
                vols = [host_volume(key, i) for i in sel]
                if shape is None:
                    shape = tuple(vols[0].shape)
                    need = 2 * n * vols[0].numel() * 4 + 2 * cls.CHUNK * vols[0].numel() * 4 + n * 8
                    free, _total = torch.cuda.mem_get_info(device)
                    if need > free:
                        raise _lib.TmfError(f"DeviceDataset: {n} subjects of {shape} need {need} bytes on {device} "
                                            f"(two float32 stores and the upload staging), {free} bytes are free")
                    for k in ("MRI", "PET"):
                        stores[k] = torch.empty((n,) + shape, device=device, dtype=torch.float32)
                for i, v in zip(sel, vols):
                    if tuple(v.shape) != shape:
                        raise _lib.TmfError(f"{what(key, i)}: shape {tuple(v.shape)} differs from {shape} of {what('MRI', 0)} "
                                            "(a DeviceDataset holds volumes of one shape)")
                raw = torch.stack(vols).to(device)
                scale_intensity_flip(raw, None, out=stores[key][c0:c0 + len(vols)])
        return cls(stores["MRI"], stores["PET"], torch.from_numpy(lab.astype(np.int64)).to(device))

    @classmethod
    def from_arrays(cls, mri, pet, labels, device="cuda") -> "DeviceDataset":
        """mri / pet: raw host volumes, numpy arrays or CPU tensors (N, 1, D, H, W) or (N, D, H, W) float32 (or sequences of
        N such volumes); labels: N integers."""
        if len(mri) != len(pet):
            raise _lib.TmfError(f"mri and pet hold {len(mri)} and {len(pet)} subjects")
        src = {"MRI": mri, "PET": pet}
        return cls._build(len(mri), lambda key, i: src[key][i], lambda key, i: f"{key}[{i}]", labels, device)

    @classmethod
    def from_nifti(cls, mri_paths: Sequence[str], pet_paths: Sequence[str], labels, device="cuda") -> "DeviceDataset":
        """One `.nii` / `.nii.gz` file per subject and modality (datasets/ADNI.py:42-46, :62), each read once."""
        from . import nifti
        if len(mri_paths) != len(pet_paths):
            raise _lib.TmfError(f"mri_paths and pet_paths hold {len(mri_paths)} and {len(pet_paths)} files")
        src = {"MRI": mri_paths, "PET": pet_paths}
        return cls._build(len(mri_paths), lambda key, i: nifti._volume_3d(src[key][i]), lambda key, i: str(src[key][i]),
                          labels, device)

    def loader(self, indices=None, batch_size: int = 1, train: bool = True, shuffle: Optional[bool] = None,
               drop_last: Optional[bool] = None, seed: Optional[int] = None, flip_prob: float = 0.3, rotate_prob: float = 0.3,
               rotate_range: float = 0.05, zoom_prob: float = 0.3, zoom_range=(0.95, 1.0)) -> DeviceLoader:
        """Batches {'MRI', 'PET' (B, 1, D, H, W) float32, 'label' int64} on the device plus the decisions drawn for them
        ('_index', '_flips', '_angles', '_zooms': numpy), over `indices` (any subset of the subjects; None = all).
        train=True: the reference's augmentation set (datasets/ADNI.py:66-68), shuffled, last short batch dropped
        (kfold_train_adversarial.py:64); train=False: ScaleIntensity only, data-set order, short last batch kept (:65-66).
        Each batch is one tmf_batch_augment launch on the current stream; the epoch's decisions are drawn at __iter__ and
        uploaded in one copy."""
        return DeviceLoader(self, indices, batch_size, train, shuffle, drop_last, seed, flip_prob, rotate_prob, rotate_range,
                            zoom_prob, zoom_range)
