"""Binding contract of the HIP extension, exercised WITHOUT a device.

Every binding validates all of its arguments on the host before it launches,
so on a CPU-only box each call below must end in a RuntimeError raised by
that validation and never in a HIP runtime error ("no ROCm-capable device",
"HIP error"), which is what a call that slipped past a missing check gives.

The module needs the built extension, and skips when a GPU is present: there
an input that slipped past a missing check would reach a kernel.
"""
import re

import pytest
import torch

import vescale_amd.ops as ops

pytestmark = [
    pytest.mark.skipif(not ops.has_ext(), reason="needs the built extension"),
    pytest.mark.skipif(torch.cuda.is_available(),
                       reason="CPU-only: with a GPU a missed check reaches a kernel"),
]

BF, F32, I64 = torch.bfloat16, torch.float32, torch.int64
PROBES = {"permlane_probe", "mfma32_probe", "tr_probe"}


def T(*shape, dtype=BF):
    """Uninitialised on purpose: no binding may get as far as reading a value,
    and no fill or conversion kernel runs (some would start the intra-op thread
    pool inside the pytest process, which the suite's fork-based multi-process
    tests do not survive)."""
    return torch.empty(*shape, dtype=dtype)


_PHILOX = ([4, 4], [4, 4], [0, 0], 0, False, 1, 0)  # gshape lshape offset flat_offset is_flat seed philox_offset
_ROPE_TAB = lambda: T(4, 4, 2, dtype=F32)  # covers S = 4, D = 8
_FA = lambda: [T(1, 2, 256, 128), T(1, 1, 256, 128), T(1, 1, 256, 128)]
_FA_BWD = lambda: _FA() + [T(1, 2, 256, 128), T(1, 2, 256, 128), T(1, 2, 256, dtype=F32)]
_FA_KV_BAD = [(1, 1, 256, 64), (1, 1, 128, 128)]
_FA_Q_BAD = [(1, 2, 256, 64), (1, 2, 128, 128)]
_FA_ARGS = {0: ("q", [(1, 2, 256, 64)]), 1: ("k", _FA_KV_BAD), 2: ("v", _FA_KV_BAD)}
_FA_BWD_ARGS = {**_FA_ARGS, 3: ("o", _FA_Q_BAD), 4: ("dout", _FA_Q_BAD),
                5: ("lse", [(1, 2, 257), (1, 2, 128)])}
_GEN = lambda: [T(1, 2, 8, 64), T(1, 1, 8, 64), T(1, 1, 8, 64)]
_GEN_ARGS = {0: ("q", []), 1: ("k", [(1, 1, 8, 32), (2, 1, 8, 64)]),
             2: ("v", [(1, 1, 9, 64), (1, 1, 4, 64)])}

# binding -> (a valid tiny call made of CPU tensors,
#             {position: (argument name, wrong shapes for that argument alone)})
# A wrong shape is one size off or a shorter operand.  An argument that
# DEFINES the call's shape (x of rmsnorm_fwd, ...) has none: any other shape
# of it is either valid or shows up as a mismatch of the arguments checked
# against it.
CASES = {
    "rmsnorm_fwd": (lambda: [T(2, 64), T(64), 1e-5],
                    {0: ("x", []), 1: ("w", [(72,), (56,)])}),
    "rmsnorm_bwd": (lambda: [T(2, 64), T(2, 64), T(64), T(2, dtype=F32), T(2, 64)],
                    {0: ("dy", []), 1: ("x", [(3, 64), (1, 64)]), 2: ("w", [(72,)]),
                     3: ("rrms", [(3,), (1,)]), 4: ("dres", [(3, 64), (1, 64)])}),
    "rmsnorm_res_fwd": (lambda: [T(2, 64), T(2, 64), T(64), 1e-5],
                        {0: ("x", []), 1: ("res", [(3, 64), (1, 64)]), 2: ("w", [(72,)])}),
    "rope": (lambda: [T(1, 4, 2, 8), _ROPE_TAB(), 0, False, False],
             {0: ("x", []), 1: ("table", [(4, 3, 2), (4, 4, 1)])}),
    "rope_qkv_fwd": (lambda: [T(1, 4, 32), _ROPE_TAB(), 1, 4, 2, 1, 8, 0],
                     {0: ("qkv", [(1, 4, 33), (1, 3, 32)]), 1: ("table", [(4, 3, 2)])}),
    "rope_qkv_bwd": (lambda: [T(1, 2, 4, 8), T(1, 1, 4, 8), T(1, 1, 4, 8), _ROPE_TAB(),
                              1, 4, 2, 1, 8, 0],
                     {0: ("dq", [(1, 2, 4, 9), (1, 1, 4, 8)]), 1: ("dk", [(1, 2, 4, 8), (1, 1, 3, 8)]),
                      2: ("dv", [(1, 2, 4, 8), (1, 1, 3, 8)]), 3: ("table", [(4, 3, 2)])}),
    "swiglu_fwd": (lambda: [T(16), T(16)], {0: ("gate", []), 1: ("up", [(17,), (8,)])}),
    "swiglu_bwd": (lambda: [T(16), T(16), T(16)],
                   {0: ("dy", []), 1: ("gate", [(17,), (8,)]), 2: ("up", [(17,), (8,)])}),
    "swiglu_packed_fwd": (lambda: [T(2, 32)], {0: ("gu", [])}),
    "swiglu_packed_bwd": (lambda: [T(2, 16), T(2, 32)],
                          {0: ("dy", [(2, 17), (1, 16)]), 1: ("gu", [])}),
    "ce_fwd": (lambda: [T(2, 64), T(2, dtype=I64), -100],
               {0: ("logits", []), 1: ("target", [(3,), (1,)])}),
    "ce_bwd": (lambda: [T(2, 64), T(2, dtype=I64), T(2, dtype=F32), T(2, dtype=F32), -100, False],
               {0: ("logits", []), 1: ("target", [(3,), (1,)]), 2: ("lse", [(3,), (1,)]),
                3: ("dloss", [(3,), (1,)])}),
    "adamw_step": (lambda: [T(16), T(16, dtype=F32), T(16), T(16, dtype=F32), T(16, dtype=F32),
                            1e-3, 0.9, 0.95, 1e-8, 0.0, 1, 1.0, T(2, dtype=F32)],
                   {0: ("param", []), 1: ("master", [(17,), (8,)]), 2: ("grad", [(17,), (8,)]),
                    3: ("m", [(17,), (8,)]), 4: ("v", [(17,), (8,)]), 12: ("clip_scale", [])}),
    "l2norm_sq": (lambda: [T(16)], {0: ("x", [])}),
    "scale_": (lambda: [T(16), T(2, dtype=F32), 1.0], {0: ("x", []), 1: ("scale_t", [])}),
    "gemm_tn": (lambda: [T(256, 64), T(256, 64), 0], {0: ("a", []), 1: ("b", [(256, 32)])}),
    "gemm_tn8": (lambda: [T(256, 64), T(256, 64), 0], {0: ("a", []), 1: ("b", [(256, 128)])}),
    "fa_fwd": (lambda: _FA() + [0.1], _FA_ARGS),
    "fa_fwd_ablate": (lambda: _FA() + [0.1, 0], _FA_ARGS),
    "fa_bwd": (lambda: _FA_BWD() + [0.1], _FA_BWD_ARGS),
    "fa_bwd2": (lambda: _FA_BWD() + [0.1, False], _FA_BWD_ARGS),
    "fa_gen_fwd": (lambda: _GEN() + [0.1, False, 0], _GEN_ARGS),
    "fa_gen_bwd": (lambda: _GEN() + [T(1, 2, 8, 64), T(1, 2, 8, 64), T(1, 2, 8, dtype=F32),
                                     T(1, 2, 8, dtype=F32), 0.1, False, 0],
                   {**_GEN_ARGS, 3: ("o", [(1, 2, 9, 64)]), 4: ("dout", [(1, 2, 9, 64), (1, 2, 4, 64)]),
                    5: ("lse", [(1, 2, 9), (1, 2, 4)]), 6: ("dlse", [(1, 2, 9)])}),
    "philox_uniform_": (lambda: [T(4, 4), *_PHILOX, 0.0, 1.0], {0: ("out", [])}),
    "philox_normal_": (lambda: [T(4, 4, dtype=F32), *_PHILOX, 0.0, 1.0], {0: ("out", [])}),
    "philox_dropout": (lambda: [T(4, 4), *_PHILOX, 0.5, True], {0: ("x", [])}),
}

# never accepted by any argument of its kind
_WRONG_DTYPE = {BF: torch.float64, F32: torch.float64, I64: torch.int32}
_DTYPE_NAME = {torch.float64: "Double", torch.int32: "Int"}


def _rejected(name, args):
    """Call the binding; it must raise from host validation, not from HIP."""
    with pytest.raises(RuntimeError) as ei:
        getattr(ops._C, name)(*args)
    msg = str(ei.value)
    assert "ROCm-capable" not in msg and "HIP error" not in msg, msg
    return msg


def test_table_covers_every_binding():
    exported = {n for n in dir(ops._C) if not n.startswith("_")}
    assert PROBES <= exported
    assert set(CASES) == exported - PROBES


@pytest.mark.parametrize("name", sorted(CASES))
def test_valid_cpu_call_is_rejected_before_the_device(name):
    make, tensors = CASES[name]
    msg = _rejected(name, make())
    first = tensors[min(tensors)][0]
    assert f"{name}: argument '{first}'" in msg and "cpu" in msg, msg


def _mutations():
    for name, (make, tensors) in sorted(CASES.items()):
        for pos, (arg, shapes) in sorted(tensors.items()):
            yield pytest.param(name, pos, arg, "dtype", None, id=f"{name}-{arg}-dtype")
            yield pytest.param(name, pos, arg, "strided", None, id=f"{name}-{arg}-strided")
            for shape in shapes:
                yield pytest.param(name, pos, arg, "shape", shape,
                                   id=f"{name}-{arg}-{'x'.join(map(str, shape))}")


@pytest.mark.parametrize("name,pos,arg,kind,shape", _mutations())
def test_one_bad_argument_is_named(name, pos, arg, kind, shape):
    args = CASES[name][0]()
    t = args[pos]
    if kind == "dtype":
        bad = T(*t.shape, dtype=_WRONG_DTYPE[t.dtype])
        fact = f"dtype={_DTYPE_NAME[bad.dtype]} "
    elif kind == "strided":
        bad = T(*t.shape, 2, dtype=t.dtype)[..., 0]
        assert bad.shape == t.shape and not bad.is_contiguous()
        fact = "contiguous=false"
    else:
        bad = T(*shape, dtype=t.dtype)
        fact = f"sizes={list(shape)} "
    args[pos] = bad
    msg = _rejected(name, args)
    assert f"{name}: argument '{arg}'" in msg, msg
    got = msg[msg.index("; got "):]
    assert fact in got, msg


def _with(name, **changes):
    """The valid call with positional arguments replaced: p<i>=value, a tuple
    standing for a bf16 tensor of that shape (f32 if it ends in F32)."""
    args = CASES[name][0]()
    for k, v in changes.items():
        if isinstance(v, tuple):
            v = T(*v[:-1], dtype=F32) if v[-1] is F32 else T(*v)
        args[int(k[1:])] = v
    return args


_PHILOX_NAMES = ("philox_uniform_", "philox_normal_", "philox_dropout")
SCALAR_RULES = (
    [("gemm_tn", dict(p2=5), "variant = 5"),
     ("gemm_tn", dict(p2=-1), "variant = -1"),
     ("gemm_tn8", dict(p2=9), "mode = 9"),
     ("fa_fwd_ablate", dict(p4=6), "mode = 6"),
     ("rope", dict(p2=1), "past the table"),
     ("rope", dict(p2=-1), "pos_offset = -1"),
     ("rope_qkv_fwd", dict(p7=1), "past the table"),
     ("rope_qkv_fwd", dict(p7=-1), "pos_offset = -1"),
     ("rope_qkv_bwd", dict(p9=1), "past the table"),
     ("rope_qkv_bwd", dict(p9=-1), "pos_offset = -1"),
     ("rope_qkv_fwd", dict(p6=7), "D = 7"),
     ("rmsnorm_fwd", dict(p0=(2, 60), p1=(60,)), "hidden"),
     ("rmsnorm_res_fwd", dict(p0=(2, 60), p1=(2, 60), p2=(60,)), "hidden"),
     ("rmsnorm_bwd", dict(p0=(2, 60), p1=(2, 60), p2=(60,), p4=(2, 60)), "hidden"),
     ("rmsnorm_bwd", dict(p0=(2, 8200), p1=(2, 8200), p2=(8200,), p4=(2, 8200)), "hidden <= 8192"),
     ("ce_fwd", dict(p0=(2, 60)), "vocab"),
     ("ce_bwd", dict(p0=(2, 60)), "vocab"),
     ("swiglu_packed_fwd", dict(p0=(2, 24)), "F2"),
     ("swiglu_packed_bwd", dict(p0=(2, 12), p1=(2, 24)), "F2"),
     ("adamw_step", dict(p10=0), "step = 0"),
     ("adamw_step", dict(p12=(0, F32)), "clip_scale"),
     ("scale_", dict(p1=(0, F32)), "scale_t"),
     ("philox_dropout", dict(p8=1.0), "p = 1"),
     ("philox_dropout", dict(p8=-0.1), "p = -0.1"),
     ("fa_fwd", dict(p0=(1, 2, 192, 128), p1=(1, 1, 192, 128), p2=(1, 1, 192, 128)), "seq = 192"),
     ("fa_fwd", dict(p0=(1, 3, 256, 128), p1=(1, 2, 256, 128), p2=(1, 2, 256, 128)), "Hq = 3"),
     ("fa_gen_fwd", dict(p5=1), "shift needs causal")]
    + [(n, dict(p2=[4]), "one length") for n in _PHILOX_NAMES]
    + [(n, dict(p3=[0]), "one length") for n in _PHILOX_NAMES]
    + [(n, dict(p1=[4] * 9, p2=[4] * 9, p3=[0] * 9), "one length") for n in _PHILOX_NAMES]
    + [(n, dict(p2=[4, 3]), "prod(lshape) = 12") for n in _PHILOX_NAMES]
)


@pytest.mark.parametrize(
    "name,changes,fact", SCALAR_RULES,
    ids=[f"{n}-{re.sub(r'[^A-Za-z0-9]+', '_', f)}-{i}" for i, (n, _, f) in enumerate(SCALAR_RULES)],
)
def test_scalar_rule(name, changes, fact):
    msg = _rejected(name, _with(name, **changes))
    assert name in msg and fact in msg, msg
