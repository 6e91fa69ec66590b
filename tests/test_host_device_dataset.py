"""Host side of the device-resident data set, no GPU: the epoch plan and its decision records in pure
numpy, the binding and argument validation of tmf_batch_augment (nothing is launched), and the kernel's resources read
from the built object."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

SHAPE = (33, 20, 29)
PROBS = dict(flip_prob=0.6, rotate_prob=0.6, rotate_range=0.05, zoom_prob=0.6, zoom_range=(0.95, 1.0))


def test_decision_record_packing():
    """One record per sample, 32 bytes, laid out as tmf_augment_decision: index, flip, do_rot, cos, sin, od, oh, ow."""
    from transmf_ad_amd import pipeline as P
    assert P.DECISION_DTYPE.itemsize == 32
    assert [P.DECISION_DTYPE.fields[n][1] for n in P.DECISION_DTYPE.names] == [0, 4, 8, 12, 16, 20, 24, 28]
    index = np.array([5, 0, 5, 2])
    flips = np.array([1, 0, 0, 1], np.uint8)
    angles = np.array([0.05, np.nan, 0.0, -0.05])
    zooms = np.array([np.nan, 0.95, 1.0, 0.9712])
    rec = P.pack_decisions(index, flips, angles, zooms, SHAPE)
    assert rec.dtype == P.DECISION_DTYPE and rec.shape == (4,) and rec.tobytes().__len__() == 128
    assert rec["index"].tolist() == [5, 0, 5, 2] and rec["flip"].tolist() == [1, 0, 0, 1]
    assert rec["do_rot"].tolist() == [1, 0, 1, 1]                     # an angle of 0.0 is still an applied rotation
    assert rec["cos_a"][0] == np.float32(math.cos(0.05)) and rec["sin_a"][3] == np.float32(math.sin(-0.05))
    assert rec["cos_a"][2] == 1.0 and rec["sin_a"][2] == 0.0 and rec["cos_a"][1] == 0.0
    sizes = [(int(r["od"]), int(r["oh"]), int(r["ow"])) for r in rec]
    assert sizes == [(0, 0, 0), (31, 19, 27), (33, 20, 29), (32, 19, 28)]     # od == 0: no zoom; zoom 1.0 is applied at full size
    # the raw words, as the kernel reads them
    words = np.frombuffer(rec.tobytes(), "<i4").reshape(4, 8)
    assert words[1].tolist()[:3] == [0, 0, 0] and words[1].tolist()[5:] == [31, 19, 27]
    assert np.frombuffer(rec.tobytes(), "<f4").reshape(4, 8)[0, 3] == np.float32(math.cos(0.05))
    with pytest.raises(P._lib.TmfError, match="zoom"):
        P.pack_decisions(index[:1], flips[:1], angles[:1], np.array([1.3]), SHAPE)


def test_shared_helpers_are_the_ones_rotate_zoom_uses():
    from transmf_ad_amd import pipeline as P
    from oracle import input_oracle as IO
    for z in (0.95, 0.9712, 0.999, 1.0):
        assert tuple(P.zoom_out_size(SHAPE, z)) == IO.zoom_out_size(SHAPE, z)
    c, s = P.rotation_cos_sin(-0.0312)
    assert c.dtype == np.float32 and c == np.float32(math.cos(-0.0312)) and s == np.float32(math.sin(-0.0312))


def test_epoch_plan_batches_tail_and_draw_order():
    """drop_last drops the tail, otherwise the last batch is short; without shuffling the order is that of `indices`; the
    decisions equal draw_decisions (the helper DevicePrefetcher draws with) batch by batch on the same RandomState, after
    the permutation when shuffling."""
    from transmf_ad_amd import pipeline as P
    idx = np.array([9, 3, 4, 7, 1, 0, 8], np.int64)
    kw = dict(PROBS)
    recs, batches = P.epoch_plan(np.random.RandomState(5), idx, 3, False, False, SHAPE, **kw)
    assert [(b["start"], b["stop"]) for b in batches] == [(0, 3), (3, 6), (6, 7)] and len(recs) == 7
    assert recs["index"].tolist() == idx.tolist()
    rs = np.random.RandomState(5)
    for b in batches:
        f, a, z = P.draw_decisions(rs, b["stop"] - b["start"], **kw)
        assert np.array_equal(b["_flips"], f) and np.array_equal(b["_angles"], a, equal_nan=True)
        assert np.array_equal(b["_zooms"], z, equal_nan=True)
        assert np.array_equal(recs[b["start"]:b["stop"]], P.pack_decisions(b["_index"], f, a, z, SHAPE))
    assert any(b["_flips"].any() for b in batches) and not all(np.isnan(b["_angles"]).all() for b in batches)

    recs, batches = P.epoch_plan(np.random.RandomState(5), idx, 3, False, True, SHAPE, **kw)
    assert [(b["start"], b["stop"]) for b in batches] == [(0, 3), (3, 6)] and recs["index"].tolist() == idx[:6].tolist()

    recs, batches = P.epoch_plan(np.random.RandomState(5), idx, 3, True, True, SHAPE, **kw)
    rs = np.random.RandomState(5)
    order = idx[rs.permutation(7)]                                   # the permutation is the first draw
    assert recs["index"].tolist() == order[:6].tolist()
    f, _a, _z = P.draw_decisions(rs, 3, **kw)
    assert np.array_equal(batches[0]["_flips"], f)

    # evaluation: nothing applied (probabilities 0), records carry the subject only
    recs, batches = P.epoch_plan(np.random.RandomState(5), idx, 4, False, False, SHAPE, 0.0, 0.0, 0.05, 0.0, (0.95, 1.0))
    assert not recs["flip"].any() and not recs["do_rot"].any() and not recs["od"].any() and len(batches) == 2
    # fewer subjects than one batch, tail dropped: an empty epoch
    recs, batches = P.epoch_plan(np.random.RandomState(5), idx[:2], 3, True, True, SHAPE, **kw)
    assert len(recs) == 0 and batches == []


def test_draw_decisions_is_the_prefetcher_stream():
    """The factored-out helper consumes a RandomState exactly as DevicePrefetcher._launch always did (restated here)."""
    from transmf_ad_amd import pipeline as P
    rs_a, rs_b = np.random.RandomState(11), np.random.RandomState(11)
    for B in (4, 1, 8):
        flips = (rs_b.random_sample(B) < 0.3).astype(np.uint8)
        angles, zooms = np.full(B, np.nan), np.full(B, np.nan)
        for b in range(B):
            if rs_b.random_sample() < 0.6:
                angles[b] = rs_b.uniform(-0.05, 0.05)
                rs_b.uniform(0.0, 0.0); rs_b.uniform(0.0, 0.0)
        for b in range(B):
            if rs_b.random_sample() < 0.6:
                zooms[b] = rs_b.uniform(0.95, 1.0)
        f, a, z = P.draw_decisions(rs_a, B, 0.3, 0.6, 0.05, 0.6, (0.95, 1.0))
        assert np.array_equal(f, flips) and np.array_equal(a, angles, equal_nan=True) and np.array_equal(z, zooms, equal_nan=True)
    assert rs_a.random_sample() == rs_b.random_sample()


def test_index_validation():
    from transmf_ad_amd import pipeline as P
    assert P.validate_indices(None, 4).tolist() == [0, 1, 2, 3]
    assert P.validate_indices([3, 0, 3], 4).dtype == np.int64
    for bad, msg in (([0, 4], "outside"), ([-1], "outside"), ([0.0, 1.0], "integers"), ([True, False], "integers"),
                     ([], "non-empty"), ([[0, 1]], "1-D")):
        with pytest.raises(P._lib.TmfError, match=msg):
            P.validate_indices(bad, 4)


def test_symbol_is_bound_and_validates_arguments():
    """tmf_batch_augment is exported and bound; a null pointer, an empty batch or store, grid limits and aliasing are
    refused with a negative code before anything is launched (the pointers here are not device memory)."""
    import ctypes as C
    from transmf_ad_amd import _lib
    lib = _lib.load()
    assert "tmf_batch_augment" in _lib.PROTOTYPES and hasattr(lib, "tmf_batch_augment")
    res, args = _lib.PROTOTYPES["tmf_batch_augment"]
    assert res is C.c_int and args == [C.c_void_p] * 7 + [C.c_int] * 5 + [C.c_void_p]
    fn = lib.tmf_batch_augment
    vol = 4 * 4 * 4 * 4
    sm, sp, lab, dec, om, op_, ol = (1 << 20) + 0 * vol, (2 << 20), (3 << 20), (4 << 20), (5 << 20), (6 << 20), (7 << 20)
    good = [sm, sp, lab, dec, om, op_, ol, 6, 2, 4, 4, 4, None]

    def rc(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return fn(*a)
    for k in range(7):
        assert rc(**{f"a{k}": None}) < 0
        assert b"NULL" in lib.tmf_last_error_string()
    for k, v in ((7, 0), (8, 0), (8, 32768), (9, 0), (9, 65536), (10, 0), (11, -1)):
        assert rc(**{f"a{k}": v}) < 0, (k, v)
    assert rc(a4=sm) < 0 and b"aliases a store" in lib.tmf_last_error_string()          # out_mri = store_mri
    assert rc(a5=sp + 5 * vol) < 0                                                         # out_pet inside store_pet (N = 6)
    assert rc(a4=sm - vol) < 0                                                             # out_mri's second sample = store_mri[0]
    assert rc(a5=om + vol) < 0 and b"alias" in lib.tmf_last_error_string()                # the two outputs overlap
    assert rc(a6=om) < 0                                                                   # labels written into a batch
    with pytest.raises(_lib.TmfError, match="tmf_batch_augment"):
        _lib.call("tmf_batch_augment", *good[:8], 0, *good[9:])


def test_batch_augment_kernel_uses_no_scratch():
    from tools import resources as R
    obj = os.path.join(R.CSRC, "input_pipeline.o")
    if not os.path.exists(obj):
        pytest.skip("objects not built (python -m transmf_ad_amd.build)")
    if not os.path.exists(f"{R.LLVM}/clang-offload-bundler"):
        pytest.skip("ROCm llvm tools not present")
    ks = [k for k in R.kernels_of(obj) if "batch_augment_kernel" in k["name"]]
    assert len(ks) == 1
    assert ks[0].get("scratch", 0) == 0 and ks[0].get("lds", 0) == 0, ks[0]
    for k in R.kernels_of(obj):                         # the kernels that now share its device functions keep theirs
        assert k.get("scratch", 0) == 0, k
