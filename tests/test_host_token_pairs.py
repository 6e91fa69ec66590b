"""Host-side argument checks (no GPU) of the three plain / _masked pairs of token entries: tmf_tok_linear_fwd,
tmf_tok_linear_bwd_input and tmf_layernorm_bwd.  Each pair shares one implementation; what an entry refuses, the code it
returns, the message it sets (its own name in it) and which check fires first are part of its contract and are listed here
call by call.  Every call in the table fails before any launch: the pointers are never touched."""
import pytest

P = 256                                          # a non-NULL, 16-byte aligned "pointer"
NULL, SHAPE = -1, -2                             # TMF_E_NULL, TMF_E_SHAPE

FWD = "tmf_tok_linear_fwd"
BWD = "tmf_tok_linear_bwd_input"
LNB = "tmf_layernorm_bwd"


def _fwd(masked, **kw):
    a = dict(x=P, w=P, bias=None, residual=None, y=P, R=16, K=64, Nout=64, ln_gamma=None, ln_beta=None, eps=1e-5,
             ln_mean=None, ln_rstd=None, ln_out=None, gelu_pre=None, mask=P)
    assert set(kw) <= set(a), kw
    a.update(kw)
    mask = a.pop("mask")
    return tuple(a.values()) + ((mask,) if masked else ()) + (None,)


def _bwd(masked, **kw):
    a = dict(dy=P, w=P, dx=P, R=16, Nout=64, K=64, gelu_pre=None, ln_x=None, ln_mean=None, ln_rstd=None, ln_gamma=None,
             add1=None, add2=None, ln_partial=None, bias_partial=None, partial_stride=0, mask=P, dx_masked=None)
    assert set(kw) <= set(a), kw
    a.update(kw)
    mask, dxm = a.pop("mask"), a.pop("dx_masked")
    return tuple(a.values()) + ((mask, dxm) if masked else ()) + (None,)


def _lnb(masked, **kw):
    a = dict(x=P, gamma=P, mean=P, rstd=P, dy=P, dx=P, partial=P, rows=16, dim=64, mask=P, dx_masked=P)
    assert set(kw) <= set(a), kw
    a.update(kw)
    mask, dxm = a.pop("mask"), a.pop("dx_masked")
    return tuple(a.values()) + ((mask, dxm) if masked else ()) + (None,)


LN_FWD = dict(ln_gamma=P, ln_beta=P, ln_mean=P, ln_rstd=P)           # a complete LayerNorm prologue
LN_BWD = dict(ln_x=P, ln_mean=P, ln_rstd=P, ln_gamma=P)              # a complete LayerNorm-backward epilogue


def _null(name):
    return NULL, f"argument '{name}' is NULL"


# (arguments, return code, substring of the message) that the plain AND the masked entry of a pair refuse alike
FWD_BOTH = [
    (dict(x=None), *_null("x")), (dict(w=None), *_null("w")), (dict(y=None), *_null("y")),
    (dict(x=None, y=None, R=0), *_null("x")),                        # pointers before shapes, in argument order
    (dict(R=0), SHAPE, "non-positive dimension"), (dict(K=0), SHAPE, "non-positive dimension"),
    (dict(Nout=-64), SHAPE, "non-positive dimension"),
    (dict(K=24), SHAPE, "K=24 must be a multiple of 16 (<= 2048) and Nout=64 a multiple of 64"),
    (dict(K=4096), SHAPE, "K=4096 must be a multiple of 16 (<= 2048)"),
    (dict(Nout=96), SHAPE, "Nout=96 a multiple of 64"),
    (dict(Nout=32), SHAPE, "Nout=32 a multiple of 64"),
    (dict(gelu_pre=P, residual=P), SHAPE, "GELU epilogue takes no residual"),
    (dict(gelu_pre=P, residual=P, K=96, **LN_FWD), SHAPE, "GELU epilogue takes no residual"),       # ... ahead of the prologue's K
    (dict(K=96, **LN_FWD), SHAPE, "the LayerNorm prologue needs K of 64, 128 or 256 (got 96)"),
    (dict(K=32, **LN_FWD), SHAPE, "(got 32)"), (dict(K=512, **LN_FWD), SHAPE, "(got 512)"),
    (dict(LN_FWD, ln_beta=None), *_null("ln_beta")), (dict(LN_FWD, ln_mean=None), *_null("ln_mean")),
    (dict(LN_FWD, ln_rstd=None), *_null("ln_rstd")),
    (dict(LN_FWD, ln_beta=None, K=96), SHAPE, "(got 96)"),           # the prologue's K ahead of its pointers
]
FWD_MASKED = [
    (dict(mask=None), *_null("mask")),
    (dict(mask=None, R=0), *_null("mask")),                          # ... ahead of the shapes
    (dict(mask=None, y=None), *_null("y")),                          # ... behind x, w, y
]
BWD_BOTH = [
    (dict(dy=None), *_null("dy")), (dict(w=None), *_null("w")), (dict(dx=None), *_null("dx")),
    (dict(R=0), SHAPE, "non-positive dimension"), (dict(Nout=0), SHAPE, "non-positive dimension"),
    (dict(K=-1), SHAPE, "non-positive dimension"),
    (dict(Nout=24), SHAPE, "Nout=24 must be a multiple of 16 (<= 2048) and K=64 a multiple of 64"),
    (dict(Nout=4096), SHAPE, "Nout=4096 must be a multiple of 16 (<= 2048)"),
    (dict(K=96), SHAPE, "K=96 a multiple of 64"),
    (dict(gelu_pre=P, bias_partial=P), SHAPE, "partial_stride must be positive"),
    (dict(LN_BWD, dx_masked=P, ln_partial=P, partial_stride=-4), SHAPE, "partial_stride must be positive"),
    (dict(bias_partial=P), SHAPE, "partial_stride must be positive"),                # ahead of every epilogue rule
    (dict(LN_BWD, dx_masked=P, ln_mean=None), *_null("ln_mean")), (dict(LN_BWD, dx_masked=P, ln_rstd=None), *_null("ln_rstd")),
    (dict(LN_BWD, dx_masked=P, ln_gamma=None), *_null("ln_gamma")),
]
BWD_PLAIN = [
    (dict(LN_BWD, K=192), SHAPE, "the LayerNorm-backward epilogue needs K of 64, 128 or 256 and no GELU (K=192)"),
    (dict(LN_BWD, K=512), SHAPE, "and no GELU (K=512)"),
    (dict(LN_BWD, gelu_pre=P), SHAPE, "and no GELU (K=64)"),         # both epilogues
    (dict(add2=P), SHAPE, "add2 needs the LayerNorm epilogue"),      # neither epilogue: add1 is the one residual it folds in
    (dict(add1=P, add2=P), SHAPE, "add2 needs the LayerNorm epilogue"),
]
BWD_MASKED = [
    (dict(gelu_pre=P, mask=None), *_null("mask")),
    (dict(mask=None, R=0), *_null("mask")),
    (dict(mask=None, dx=None), *_null("dx")),
    (dict(LN_BWD, gelu_pre=P, dx_masked=P), SHAPE, "needs exactly one of the GELU-gradient and LayerNorm-backward epilogues"),
    (dict(), SHAPE, "needs exactly one"), (dict(add1=P), SHAPE, "needs exactly one"), (dict(add2=P), SHAPE, "needs exactly one"),
    (dict(LN_BWD, dx_masked=P, K=192), SHAPE, "the LayerNorm-backward epilogue needs K of 64, 128 or 256 (K=192)"),
    (dict(LN_BWD, K=192), SHAPE, "256 (K=192)"),                     # K ahead of the epilogue's pointers
    (dict(LN_BWD), *_null("dx_masked")),
    (dict(LN_BWD, ln_gamma=None), *_null("ln_gamma")),               # ... and dx_masked behind the other three
    (dict(gelu_pre=P, add1=P), SHAPE, "the GELU-gradient epilogue takes no add1, add2 or dx_masked"),
    (dict(gelu_pre=P, add2=P), SHAPE, "takes no add1, add2 or dx_masked"),
    (dict(gelu_pre=P, dx_masked=P), SHAPE, "takes no add1, add2 or dx_masked"),
]
LNB_BOTH = [(dict([(n, None)]), *_null(n)) for n in ("x", "gamma", "mean", "rstd", "dy", "dx", "partial")] + [
    (dict(dx=None, rows=0), *_null("dx")),
    (dict(rows=0), SHAPE, "rows=0 dim=64"), (dict(dim=0), SHAPE, "rows=16 dim=0"), (dict(rows=-3, dim=4096), SHAPE, "rows=-3"),
    (dict(dim=4096), SHAPE, "dim=4096 exceeds 2048"), (dict(dim=2052), SHAPE, "dim=2052 exceeds 2048"),
    (dict(dim=513), SHAPE, "dim=513 exceeds 512"),                   # not a multiple of 4: one float per lane and group
]
LNB_MASKED = [
    (dict(mask=None), *_null("mask")), (dict(dx_masked=None), *_null("dx_masked")),
    (dict(mask=None, dx_masked=None), *_null("mask")), (dict(mask=None, partial=None), *_null("partial")),
    (dict(dx_masked=None, rows=0), *_null("dx_masked")),
]

CASES = []
for base, args, both, plain, masked in ((FWD, _fwd, FWD_BOTH, [], FWD_MASKED), (BWD, _bwd, BWD_BOTH, BWD_PLAIN, BWD_MASKED),
                                        (LNB, _lnb, LNB_BOTH, [], LNB_MASKED)):
    for m, rows in ((False, both + plain), (True, both + masked)):
        for kw, rc, text in rows:
            entry = base + ("_masked" if m else "")
            CASES.append(pytest.param(entry, args(m, **kw), rc, text, id=f"{entry}-{len(CASES)}"))


@pytest.mark.parametrize("entry,args,rc,text", CASES)
def test_invalid_call(entry, args, rc, text):
    from transmf_ad_amd import _lib
    assert len(args) == len(_lib.PROTOTYPES[entry][1])
    with pytest.raises(_lib.TmfError) as e:
        _lib.call(entry, *args)
    msg = str(e.value)
    assert msg.startswith(f"{entry} failed (rc={rc}): {entry}: "), msg         # the entry's own name, never a helper's
    assert text in msg, msg
    assert msg.count("tmf_") == 2, msg                                        # ... and no second name further in


# ---------------------------------------------------------------------------------------------------------------------
# the two one-call forward entries check their arguments in one place (csrc/fusion_path.hip: check_fwd_args); the name of
# the workspace argument in the messages is the entry's own
# ---------------------------------------------------------------------------------------------------------------------
ALIGN, WORKSPACE = -3, -4                        # TMF_E_ALIGN, TMF_E_WORKSPACE
FUSION_FWD = [("tmf_fusion_train_fwd", "saved", "saved workspace 0 B < required"),
              ("tmf_fusion_infer_fwd", "workspace", "workspace 0 B < required")]
# (desc overrides, mri_tok, pet_tok, inst given, workspace, cls) -> code, message after the entry's name ({ws}: see above)
FUSION_ROWS = [
    (dict(), None, P, True, P, P, NULL, "argument 'mri_tok' is NULL"),
    (dict(), P, None, True, P, P, NULL, "argument 'pet_tok' is NULL"),
    (dict(), P, P, True, None, P, NULL, "argument '{ws}' is NULL"),
    (dict(), P, P, True, P, None, NULL, "argument 'cls' is NULL"),
    (dict(), P, None, True, None, None, NULL, "argument 'pet_tok' is NULL"),           # in argument order
    (dict(), P, P, False, P, P, NULL, "argument 'inst' is NULL"),
    (dict(), P, P, False, P, None, NULL, "argument 'cls' is NULL"),                    # cls ahead of inst
    (dict(), P + 4, P, True, P, P, ALIGN, "argument 'mri_tok' is not 16-byte aligned"),
    (dict(), P, P + 8, True, P, P, ALIGN, "argument 'pet_tok' is not 16-byte aligned"),
    (dict(), P, P, True, P + 4, P, ALIGN, "argument '{ws}' is not 16-byte aligned"),
    (dict(), P + 4, P, False, P, P, NULL, "argument 'inst' is NULL"),                  # every NULL ahead of the alignment
    (dict(dim=96), None, P, True, P, P, SHAPE, "needs dim of 64, 128 or 256"),         # the descriptor ahead of the pointers
    (dict(), P, P, True, P, P, WORKSPACE, "{size}"),                                   # the size after all of them
]


@pytest.mark.parametrize("entry,ws,size", FUSION_FWD)
@pytest.mark.parametrize("row", range(len(FUSION_ROWS)))
def test_fusion_forward_entries_refuse_alike(entry, ws, size, row):
    import ctypes
    from transmf_ad_amd import _lib
    over, mri, pet, with_inst, wsp, cls, rc, text = FUSION_ROWS[row]
    d = dict(B=2, N=5, dim=64, heads=4, dim_head=16, mlp=64, depth=1, flags=0)
    d.update(over)
    inst = (_lib.XformerParams * 2)() if with_inst else None
    with pytest.raises(_lib.TmfError) as e:
        _lib.call(entry, ctypes.byref(_lib.FusionDesc(**d)), mri, pet, inst, wsp, 0, cls, None)
    msg = str(e.value)
    assert msg.startswith(f"{entry} failed (rc={rc}): {entry}: " + text.format(ws=ws, size=size)), msg
