"""The ctypes binding is derived from include/tmf_hip.h (transmf_ad_amd/_lib.py parse_header): the struct layouts and the
constants against what the host C compiler makes of the same header, argument lists of the entries that are hard to
parse against expectations written here by hand, and the parser's refusal of what it cannot map.  No GPU needed."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from transmf_ad_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I, F, D, L, Z = C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_long, C.c_size_t


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """{text: number} printed by a C program generated from the parsed structs and constants and compiled against the
    header: "sizeof S", "offsetof S.f", "sizeof S.f", "TMF_X", "TMF_SNET_ALGO_WINO(m)".  The compiler is the reference."""
    cc = next((c for c in (shutil.which("cc"), shutil.which("gcc"), shutil.which("clang")) if c), None)
    if cc is None:
        pytest.skip("no host C compiler")
    lines = []
    for cname, cls in _lib.STRUCTS.items():
        lines.append(f'printf("sizeof {cname} %zu\\n", sizeof({cname}));')
        for f, _t in cls._fields_:
            lines.append(f'printf("offsetof {cname}.{f} %zu\\n", offsetof({cname}, {f}));')
            lines.append(f'printf("sizeof {cname}.{f} %zu\\n", sizeof((({cname}*)0)->{f}));')
    lines += [f'printf("{n} %lld\\n", (long long)({n}));' for n in _lib.CONSTANTS]
    lines += [f'printf("TMF_SNET_ALGO_WINO({m}) %lld\\n", (long long)TMF_SNET_ALGO_WINO({m}));' for m in range(4)]
    d = tmp_path_factory.mktemp("abi")
    src = d / "abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tmf_hip.h"\nint main(void) {\n' + "\n".join(lines)
                   + "\nreturn 0;\n}\n")
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(d / "abi"), str(src)], check=True, capture_output=True,
                   timeout=120)
    out = subprocess.run([str(d / "abi")], check=True, capture_output=True, text=True, timeout=60).stdout
    return {k: int(v) for k, v in (line.rsplit(" ", 1) for line in out.splitlines())}


def test_struct_layouts_match_the_c_compiler(compiled):
    assert len(_lib.STRUCTS) == 13
    for cname, cls in _lib.STRUCTS.items():
        assert C.sizeof(cls) == compiled[f"sizeof {cname}"], cname
        assert len(cls._fields_) >= 1
        for f, _t in cls._fields_:
            assert getattr(cls, f).offset == compiled[f"offsetof {cname}.{f}"], (cname, f)
            assert getattr(cls, f).size == compiled[f"sizeof {cname}.{f}"], (cname, f)
    # the classes keep their names as module attributes, the name tuples follow the structs
    assert _lib.STRUCTS["tmf_snet_desc"] is _lib.SnetDesc and _lib.STRUCTS["tmf_heads_cnn_params"] is _lib.HeadsCnnParams
    assert _lib.SnetDesc._fields_[7] == ("momentum", F * 7) and _lib.SnetGrads._fields_[-1] == ("deep_event", P)
    assert _lib.HEADS_PARAMS == tuple(n for n, _t in _lib.HeadsGrads._fields_) and len(_lib.HEADS_PARAMS) == 16
    assert _lib.HEADS_BUFFERS == ("bn1_rm", "bn1_rv", "bn5_rm", "bn5_rv", "dbn_rm", "dbn_rv")
    assert _lib.HEADS_CNN_PARAMS == ("fc0_w", "fc0_b", "fc2_w", "fc2_b", "d0_w", "d0_b", "dbn_g", "dbn_b", "d3_w", "d3_b")
    assert [n for n, _t in _lib.HeadsCnnParams._fields_][8:10] == ["dbn_rm", "dbn_rv"]        # ahead of d3_*
    assert _lib.XFORMER_PTRS == ("ln1_g", "ln1_b", "wq", "wkv", "wo", "bo", "ln2_g", "ln2_b", "w1", "b1", "w2", "b2", "lnf_g", "lnf_b")


def test_constants_equal_their_defines(compiled):
    assert len(_lib.CONSTANTS) >= 34
    for name, value in _lib.CONSTANTS.items():
        assert name.startswith("TMF_") and compiled[name] == value == getattr(_lib, name[4:]), name
    for m in range(4):
        assert _lib.snet_algo_wino(m) == compiled[f"TMF_SNET_ALGO_WINO({m})"]
    assert (_lib.POOL_NONE, _lib.POOL_MAX2, _lib.POOL_AVG2, _lib.DW_REFERENCE, _lib.SNET_ALONE, _lib.SNET_DEEP_FROM) == (0, 1, 2, 1, 1, 3)
    assert (_lib.MASK_SEGMENTS, _lib.FUSION_PER_OP, _lib.ADAM_MAX_TENSORS, _lib.TRAIN_METRICS_WORDS) == (20, 1, 160, 8)
    assert _lib.PRECISION == {"fp32": 0, "bf16": 1, "fp32x": 2} and _lib.E_ARG == -5
    assert [_lib.pool_code(p) for p in (None, "none", "max", "avg")] == [0, 0, 1, 2]


def test_hard_to_parse_prototypes():
    pr = _lib.PROTOTYPES
    assert pr["tmf_bn_finalize"] == (I, [P, I, I, D, P, P, P, P, P, F, F, P, P, P, P, P])
    assert pr["tmf_dropout_keep_masks"] == (I, [I, P, P, P, C.c_ulonglong, C.c_ulonglong, P])
    assert pr["tmf_set_option"] == (I, [C.c_char_p, I])
    assert pr["tmf_last_error_string"] == (C.c_char_p, []) and pr["tmf_version"] == (I, [])
    assert pr["tmf_adam_state_elems"] == (L, [I, P])
    assert pr["tmf_adam_step"] == (I, [I, P, P, P, P, P, D, D, D, D, D, I, P])
    assert pr["tmf_debug_xf_trace"] == (None, [P, P, P])
    assert pr["tmf_eval_metrics_update"] == (I, [P, P, P, L, P, P, I, I, P])
    sd, sp, sg = (C.POINTER(s) for s in (_lib.SnetDesc, _lib.SnetParams, _lib.SnetGrads))
    assert pr["tmf_snet_train_fwd"] == (I, [sd, P, sp, P, Z, P, P])
    assert pr["tmf_snet_train_bwd_input"] == (I, [sd, P, P, Z, P, sg, P, Z, P, P])
    assert pr["tmf_snet_saved_bytes"] == (Z, [sd])
    assert pr["tmf_fusion_train_bwd"][1][3] == C.POINTER(_lib.XformerParams) and pr["tmf_fusion_train_bwd"][1][7] == C.POINTER(_lib.XformerGrads)
    assert pr["tmf_batch_augment"][1][3] is P                     # tmf_augment_decision*: records in device memory
    assert pr["tmf_conv3d_wgrad_wino_tiles"] == (L, [I] * 6) and pr["tmf_conv3d_fwd_kernel_name"] == (C.c_char_p, [I] * 7)
    assert pr["tmf_conv_block_algo"] == (I, [I] * 4)
    assert pr["tmf_conv3d_wgrad_bf16_plan"] == (I, [I] * 7 + [P, P])              # int* results: host pointers
    with pytest.raises(C.ArgumentError):                          # a wrong struct still raises
        _lib.load().tmf_snet_saved_bytes(C.byref(_lib.FusionDesc()))


_GOOD = "#define TMF_N 3\ntypedef struct tmf_s { int a; float v[TMF_N]; const float *p, *q; } tmf_s;\nint tmf_f(const tmf_s* d, long n, void* stream);\n"


@pytest.mark.parametrize("text, names", [
    ("int tmf_f(const foo_t* x, int n);", ("tmf_hip.h:4:", "tmf_f", "foo_t")),                # unknown pointer type
    ("\n\nint tmf_f(unsigned n);", ("tmf_hip.h:6:", "tmf_f", "unsigned")),                  # unknown scalar type
    ("/* c */\nint tmf_f(int, float* y);", ("tmf_hip.h:5:", "tmf_f", "unnamed", "int")),      # unnamed parameter
    ("int tmf_f(const float*);", ("tmf_f", "unnamed")),
    ("typedef struct tmf_t { float v[NBLK]; } tmf_t;", ("tmf_hip.h:4:", "tmf_t", "NBLK")),    # unknown array size
    ("typedef struct tmf_t { short v; } tmf_t;", ("tmf_t", "short")),                         # unknown field type
    ("int tmf_f(void (*cb)(int), int n);", ("tmf_hip.h:4:", "not a function declaration")),   # function pointer
    ("int tmf_a(int n), tmf_b(int n);", ("not a function declaration",)),                     # two declarations per ;
    ("short tmf_f(int n);", ("tmf_f", "short")),                                              # unknown return type
    ("#define TMF_X (1 << 3)\n", ("TMF_X",)),                                                 # a define that is no integer literal
])
def test_parser_refuses_what_it_cannot_map(text, names):
    """(_GOOD is three lines: the refused text starts on line 4.)"""
    with pytest.raises(_lib.HeaderError) as e:
        _lib.parse_header(_GOOD + text)
    for n in names:
        assert n in str(e.value), (n, str(e.value))


def test_parser_reads_the_conventions():
    consts, structs, protos = _lib.parse_header(_GOOD)
    assert consts == {"TMF_N": 3}
    s = structs["tmf_s"]
    assert s.__name__ == "S" and s._fields_ == [("a", I), ("v", F * 3), ("p", P), ("q", P)]
    assert protos == {"tmf_f": (I, [C.POINTER(s), L, P])}
