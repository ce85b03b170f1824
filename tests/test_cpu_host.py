"""CPU-side checks of the host layer: C-ABI library exports, drop-in module API / state-dict keys,
and loud failure (no silent CPU fallback)."""
import contextlib
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import aanet_amd
from aanet_amd import _lib, nets, ops
from tests.golden_io import golden, state_dict_of

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    txt = open(os.path.join(REPO, "include", "aanet_mi355x.h")).read()
    return sorted(set(re.findall(r"\b(aanet_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_header_symbol():
    L = ctypes.CDLL(_lib.LIB_PATH)
    fns = header_functions()
    assert len(fns) >= 15
    for f in fns:
        assert hasattr(L, f), f"{f} declared in include/aanet_mi355x.h but not exported"
    assert set(fns) == set(_lib.exported_symbols())


def header_prototypes():
    """{name: (return kind, [parameter kinds])} of every aanet_* prototype in the header, comments
    stripped.  Kinds: "ptr" (anything with a * or an aanet_stream_t), "int", "long", "float",
    "size_t"."""
    txt = open(os.path.join(REPO, "include", "aanet_mi355x.h")).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    txt = re.sub(r"//[^\n]*", " ", txt)

    def kind(decl, what):
        decl = " ".join(decl.split())
        if "*" in decl or re.search(r"\baanet_stream_t\b", decl):
            return "ptr"
        words = [w for w in re.findall(r"[A-Za-z_]\w*", decl) if w not in ("const", "unsigned")]
        for k in ("size_t", "long", "int", "float"):
            if words and words[0] == k:
                return k
        raise AssertionError(f"{what}: cannot classify '{decl}'")

    protos = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w \t\n]*?[\s*]+)(aanet_[a-z0-9_]+)\s*\(([^()]*)\)\s*;",
                                        txt):
        assert name not in protos, f"{name} declared twice"
        params = params.strip()
        plist = [] if params in ("", "void") else [kind(p, name) for p in params.split(",")]
        protos[name] = (kind(ret, name), plist)
    return protos


_CTYPE_KIND = {ctypes.c_void_p: "ptr", ctypes.c_char_p: "ptr", ctypes.c_int: "int",
               ctypes.c_long: "long", ctypes.c_float: "float", ctypes.c_size_t: "size_t"}


def test_ctypes_argument_lists_match_the_header():
    """Every aanet_* prototype's parameter kinds, in order, equal the ctypes argtypes the package
    binds for that name (_lib._SIGNATURES, _lib._SIZE_FUNCTIONS, aanet_status_string in
    _lib.lib()), and the return kinds agree.  An int that became a long, or an argument added on
    one side only, shifts every later argument without any symbol name changing."""
    # ctypes.c_size_t is an alias of c_ulong here: distinguish by identity first, and make sure the
    # table cannot mistake a long for a size_t
    assert ctypes.c_size_t is not ctypes.c_long and ctypes.c_int is not ctypes.c_long
    protos = header_prototypes()
    assert set(protos) == set(header_functions())
    bound = {name: ("int", argtypes) for name, argtypes in _lib._SIGNATURES.items()}
    for name, argtypes, restype in _lib._SIZE_FUNCTIONS:
        assert name not in bound
        bound[name] = (_CTYPE_KIND[restype], argtypes)
    L = _lib.lib()
    bound["aanet_status_string"] = (_CTYPE_KIND[L.aanet_status_string.restype],
                                    list(L.aanet_status_string.argtypes))
    assert set(bound) == set(protos)
    assert len(protos) >= 63
    for name, (ret, params) in sorted(protos.items()):
        bret, argtypes = bound[name]
        assert [_CTYPE_KIND[a] for a in argtypes] == params, \
            f"{name}: header {params} != ctypes {[_CTYPE_KIND[a] for a in argtypes]}"
        assert bret == ret, f"{name}: header returns {ret}, bound as {bret}"
        # and what lib() actually set on the loaded symbol is that list
        f = getattr(L, name)
        assert list(f.argtypes or []) == list(argtypes), name
        assert _CTYPE_KIND[f.restype] == ret, name
    # the parser itself, on the prototypes whose kinds are least uniform
    p = protos
    assert p["aanet_version"] == ("int", [])
    assert p["aanet_status_string"] == ("ptr", ["int"])
    assert p["aanet_conv_weight_pack_split_bytes"] == ("long", ["int"] * 5)
    assert p["aanet_conv3x3s2_pack_bytes"] == ("size_t", ["int", "int"])
    assert p["aanet_mdcn_fwd_fused_f32"][1][:7] == ["ptr", "ptr", "long", "ptr", "long", "int", "float"]
    assert p["aanet_resize_bilinear_f32"][1] == ["ptr", "ptr", "long"] + ["int"] * 4 + ["ptr"]
    assert p["aanet_mdcn_bwd_algo_f32"][1][-3:] == ["ptr", "size_t", "ptr"]


def test_library_version_and_status_strings():
    L = _lib.lib()
    assert L.aanet_version() == _lib.ABI_VERSION == 4
    assert b"struct_size" in L.aanet_status_string(_lib.EABI)
    assert L.aanet_status_string(0) == b"ok"
    assert L.aanet_status_string(-1) == b"invalid argument"
    assert L.aanet_status_string(-2) == b"unsupported configuration"


def test_invalid_arguments_are_rejected_without_a_gpu():
    """Argument validation runs on the host before any launch: bad sizes return AANET_EINVAL."""
    L = _lib.lib()
    assert L.aanet_corr_volume_f32(None, None, None, 1, 1, 1, 1, 1, None) == -1
    assert L.aanet_disp_regress_f32(None, None, 0, 1, 1, 1, 0, None) == -1
    # C not divisible by groups
    args = [None] * 6 + [1, 3, 4, 4, 4, 3, 3, 1, 1, 1, 2, 1, None]
    assert L.aanet_mdcn_fwd_f32(*args) == -1
    with pytest.raises(_lib.AanetError):
        _lib.call("aanet_corr_volume_f32", None, None, None, 0, 1, 1, 1, 1, None)


def test_conv_fused_null_arguments_rejected_before_the_direct_kernel():
    """aanet_conv2d_fused_f32 on a few-channel shape (3 -> 32, 7x7 / 3: the direct VALU kernel of
    small_conv.hip) with a null x / weight / out, or post_scale without post_shift, returns
    AANET_EINVAL on the host instead of launching (the direct dispatch ran before the
    engine's checks).  No GPU is touched: the checks come first."""
    import ctypes as C
    L = _lib.lib()
    f = L.aanet_conv2d_fused_f32
    buf = (C.c_float * 4)()
    p = C.cast(buf, C.c_void_p)
    shape = [1, 3, 48, 96, 32, 7, 7, 3, 2, 1, 1, 0, None]  # n c h w co kh kw s pad dil g layout st
    for x, w, out, ps, sh in ((None, p, p, None, None), (p, None, p, None, None),
                              (p, p, None, None, None), (p, p, p, p, None)):
        assert f(x, w, None, ps, sh, None, 1, 0, out, *shape) == -1


def test_descriptor_size_is_checked_without_a_gpu():
    """Descriptor structs carry struct_size (ABI version 4): a caller built against another
    header layout gets AANET_EABI before anything is read past the struct or launched (ADVICE r3:
    a version-1 caller passed the smaller aanet_csa_epilogue_t and the library read `post` past
    its end)."""
    import ctypes as C
    L = _lib.lib()
    d = _lib.CsaEpilogue()
    assert d.struct_size == C.sizeof(_lib.CsaEpilogue)
    assert _lib.PostStage().struct_size == C.sizeof(_lib.PostStage)
    assert _lib.S2Terms(None, 0).struct_size == C.sizeof(_lib.S2Terms)
    dummy = C.c_void_p(16)  # never dereferenced: the descriptor check comes first
    args = lambda desc: ([None] * 5 + [0, dummy, None, None, 0, 64, None, 1, 64, 8, 8, 64, 3, 3, 1, 1, 1]  # noqa: E731
                         + [C.byref(desc), 1, None])
    d.struct_size -= 8  # the version-1 layout had no `post` pointer
    assert L.aanet_conv2d_pw_f32(*args(d)) == _lib.EABI
    d.struct_size += 8
    p = _lib.PostStage()
    p.struct_size = 8
    d.post = C.pointer(p)
    assert L.aanet_conv2d_pw_f32(*args(d)) == _lib.EABI
    t = _lib.S2Terms(None, 0)
    t.struct_size = 0
    assert L.aanet_conv3x3s2_terms_f32(None, None, None, 1, 32, 8, 8, 16, 16, None, 0, None, 0,
                                       C.byref(t), None) == _lib.EABI


def test_corr_volume_bwd_refuses_its_lds_limit_without_a_gpu():
    """aanet_corr_volume_bwd_f32 stages 4 (D + 8)(64 + 2 (D - 1)) bytes of grad_out in LDS: D = 124
    is the last size within the CU's 160 KiB (162,096 B), D = 125 (165,312 B) must come back as
    AANET_EUNSUPPORTED from the host check, before anything is launched (the pointers are dummies
    that a launch would fault on), and as an AanetError through _lib.call.  Catches a launcher
    that drops the refusal or moves it behind the launch."""
    import ctypes as C
    L = _lib.lib()
    assert 4 * (124 + 8) * (64 + 2 * 123) <= 160 * 1024 < 4 * (125 + 8) * (64 + 2 * 124)
    p = C.c_void_p(16)  # never dereferenced: the size check comes first
    args = (p, p, p, p, p, 1, 4, 1, 64, 125, None)
    assert L.aanet_corr_volume_bwd_f32(*args) == _lib.EUNSUPPORTED
    with pytest.raises(_lib.AanetError) as e:
        _lib.call("aanet_corr_volume_bwd_f32", *args)
    assert e.value.status == _lib.EUNSUPPORTED


def test_conv3x3s2_terms_refuses_an_oversized_up_tensor_without_a_gpu():
    """aanet_conv3x3s2_terms_f32 reads the resized CSA term through a per-image buffer resource
    with 32-bit sizes (co_a * up_h * up_w * 4 bytes): an `up` of 2^31 bytes or more per image must
    be AANET_EUNSUPPORTED like the other three tensors' bounds, on the host (dummy pointers).
    Catches a launcher whose resource size wraps and lets every `up` load fall out of range."""
    import ctypes as C
    L = _lib.lib()
    p = C.c_void_p(16)
    # 16 channels x 8192 x 4096 floats = 2^31 bytes, the first size refused
    big = _lib.S2Terms(None, 0, None, p, 8192, 4096)
    args = lambda t: (p, p, None, 1, 32, 8, 8, 16, 16, p, 0, None, 0, C.byref(t), None)  # noqa: E731
    assert L.aanet_conv3x3s2_terms_f32(*args(big)) == _lib.EUNSUPPORTED
    with pytest.raises(_lib.AanetError) as e:
        _lib.call("aanet_conv3x3s2_terms_f32", *args(big))
    assert e.value.status == _lib.EUNSUPPORTED
    # up_h = 0 stays an invalid argument (checked before the size)
    assert L.aanet_conv3x3s2_terms_f32(*args(_lib.S2Terms(None, 0, None, p, 0, 4096))) == -1


def test_import_leaves_global_torch_flags_alone():
    """importing the package no longer turns TF32 off process-wide; the package's module
    forwards switch it off for their own MIOpen convs and restore it."""
    import subprocess
    import sys
    code = ("import torch; a = torch.backends.cudnn.allow_tf32; import aanet_amd; "
            "from aanet_amd._precision import fp32_convs; "
            "seen = []; f = fp32_convs(lambda: seen.append(torch.backends.cudnn.allow_tf32)); f(); "
            "print(a, torch.backends.cudnn.allow_tf32, seen[0])")
    out = subprocess.run([sys.executable, "-c", code], cwd=REPO, capture_output=True, text=True,
                         timeout=120).stdout.split()
    assert out == ["True", "True", "False"], out


def test_fp32_scope_covers_the_conv_backward():
    """autograd's conv backward reads the global TF32 flag at loss.backward(), outside
    the decorated forward.  fp32_scope (what Trainer runs its step in) keeps it off there too; a
    bare decorated forward alone does not (the documented reason for the scope)."""
    from aanet_amd._precision import fp32_convs, fp32_scope
    conv = torch.nn.Conv2d(2, 2, 3)
    fwd = fp32_convs(lambda x: conv(x))
    prev = torch.backends.cudnn.allow_tf32
    torch.backends.cudnn.allow_tf32 = True
    try:
        for scoped in (True, False):
            seen = []
            h = conv.weight.register_hook(lambda g: seen.append(torch.backends.cudnn.allow_tf32))
            ctx = fp32_scope() if scoped else contextlib.nullcontext()
            with ctx:
                fwd(torch.randn(1, 2, 5, 5)).sum().backward()
            h.remove()
            assert seen == [not scoped], (scoped, seen)
            assert torch.backends.cudnn.allow_tf32 is True
    finally:
        torch.backends.cudnn.allow_tf32 = prev


def test_ops_fail_loudly_on_cpu_tensors():
    x = torch.zeros(1, 4, 3, 5)
    with pytest.raises(NotImplementedError):
        ops.corr_volume(x, x, 2)
    with pytest.raises(NotImplementedError):
        nets.DisparityEstimation(4)(torch.zeros(1, 4, 3, 5))
    with pytest.raises(NotImplementedError):
        nets.ModulatedDeformConv(4, 4, 3, padding=1)(x, torch.zeros(1, 18, 3, 5), torch.ones(1, 9, 3, 5))


@pytest.mark.parametrize("inter", [True, False])
def test_state_dict_keys_match_reference(inter):
    g = golden("aggregation_inter" if inter else "aggregation_final")
    ref = state_dict_of(g)
    m = nets.AdaptiveAggregation(16, num_scales=3, num_fusions=6, num_stage_blocks=1,
                                 num_deform_blocks=3, intermediate_supervision=inter)
    ours = m.state_dict()
    assert set(ours) == set(ref)
    for k, v in ref.items():
        assert tuple(ours[k].shape) == v.shape, k


def test_hot_path_module_api_mirrors_aanet():
    m = nets.AANetHotPath(64, no_intermediate_supervision=True)
    # AANet eval config (max_disp=192 -> 64): final fusion has one output branch, one final conv
    assert len(m.aggregation.final_conv) == 1
    assert len(m.aggregation.fusions[-1].fuse_layers) == 1
    assert isinstance(m.cost_volume, nets.CostVolumePyramid)
    # the DCN-bearing keys the training LR grouping relies on (utils/utils.py:156-169)
    keys = list(m.state_dict())
    assert any(k.endswith("conv2.offset_conv.weight") for k in keys)
    assert any(k.endswith("conv2.deform_conv.weight") for k in keys)
    w = m.state_dict()["aggregation.fusions.5.branches.0.0.conv2.offset_conv.weight"]
    assert tuple(w.shape) == (54, 32, 3, 3)
    # offset_conv is zero-initialised like the reference (deform.py:74-76)
    assert float(w.abs().sum()) == 0.0


def test_package_exposes_native_library_path():
    assert aanet_amd.native_library_path().endswith("libaanet_mi355x.so")
    assert os.path.exists(aanet_amd.native_library_path())


def test_torch_ops_registered_and_refuse_cpu():
    """torch.ops.aanet.* exist (SURVEY §8b op-level API), shape-propagate through fake kernels,
    and have no CPU kernel (the reference DCN is CUDA-only)."""
    import torch
    import aanet_amd  # noqa: F401  (registers the ops)
    from aanet_amd.torch_ops import OPS
    for name in OPS:
        assert hasattr(torch.ops.aanet, name), name
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        x = torch.empty(2, 8, 10, 12)
        w = torch.empty(6, 8, 3, 3)
        off, msk = torch.empty(2, 18, 10, 12), torch.empty(2, 9, 10, 12)
        y = torch.ops.aanet.mdcn_forward(x, off, msk, w, None, 1, 2, 2, 1, 1)
        assert tuple(y.shape) == (2, 6, 10, 12)
        v = torch.ops.aanet.corr_volume(x, x, 5)
        assert tuple(v.shape) == (2, 5, 10, 12)
        assert tuple(torch.ops.aanet.disp_regress(v, False).shape) == (2, 10, 12)
    with pytest.raises(NotImplementedError):
        torch.ops.aanet.corr_volume(torch.randn(1, 4, 3, 5), torch.randn(1, 4, 3, 5), 2)


def test_mdcn_backward_workspace_sizes():
    """aanet_mdcn_bwd_ws_workspace_size: the NHWC grad_x accumulator + channels-last x + W^T
    (>= 2*n*c*h*w + co*c*k floats); the deterministic layout holds its int64 accumulators too,
    per chunk of images; invalid shapes give 0."""
    L = _lib.lib()
    n, c, h, w, co = 2, 64, 12, 30, 64
    args = (n, c, h, w, co, 3, 3, 1, 2, 2, 1, 2)
    ws = L.aanet_mdcn_bwd_ws_workspace_size(*args)
    det = L.aanet_mdcn_bwd_det_workspace_size(*args)
    assert ws >= 4 * (2 * n * c * h * w + co * c * 9)
    assert det >= 8 * n * c * h * w + 4 * (n * c * h * w + co * c * 9)
    assert L.aanet_mdcn_bwd_ws_workspace_size(n, 63, h, w, co, 3, 3, 1, 2, 2, 1, 2) == 0  # C % dg
    # the window form's int64 weight-gradient accumulator (co*c*9 int64) is present
    assert det >= 8 * n * c * h * w + 4 * n * c * h * w + 8 * co * c * 9
    # the deterministic backward runs in chunks of images (96 MB of int64 grad_x + channels-last
    # x each): the workspace stops growing with the batch -- agg_s0 (64 channels, 128 x 416) at
    # B = 8 and B = 64 takes the same <= 128 MB (round 4: ~0.9 GB at B = 8)
    agg = (64, 128, 416, 64, 3, 3, 1, 2, 2, 1, 2)
    d8 = L.aanet_mdcn_bwd_det_workspace_size(8, *agg)
    d64 = L.aanet_mdcn_bwd_det_workspace_size(64, *agg)
    assert d8 == d64 and d8 <= 128 << 20
    assert d8 >= 12 * 2 * 64 * 128 * 416  # two images per chunk
    assert L.aanet_mdcn_bwd_det_workspace_size(1, *agg) < d8


def test_window_fwd_support_query_without_a_gpu():
    """aanet_mdcn_window_fwd_supported (the op-level DCN forward's window dispatch) takes exactly
    the aggregation's deformable convs: 3x3, stride 1, pad = dil = 2, one conv group, two
    deformable groups, C = Co in {32, 64, 128}, W % 4 == 0 (nets/deform.py:216-226; 128 channels:
    SURVEY C4's feat_s1 shape)."""
    ok = ops.window_fwd_ok
    assert ok(64, 64, 3, 3, 1, 2, 2, 1, 2, 416) and ok(32, 32, 3, 3, 1, 2, 2, 1, 2, 208)
    assert ok(128, 128, 3, 3, 1, 2, 2, 1, 2, 104)
    assert not ok(16, 16, 3, 3, 1, 2, 2, 1, 2, 104)      # scale 2: 8 channels per group
    assert not ok(128, 128, 3, 3, 1, 1, 1, 1, 2, 104)    # feature DCN
    assert not ok(64, 64, 3, 3, 2, 2, 2, 1, 2, 416)      # stride 2
    assert not ok(64, 64, 3, 3, 1, 2, 2, 1, 2, 26)       # W % 4
    assert not ok(64, 32, 3, 3, 1, 2, 2, 1, 2, 416)      # Co != C
    assert not ok(64, 64, 3, 3, 1, 2, 2, 2, 2, 416)      # conv groups
    assert not ok(64, 64, 3, 3, 1, 1, 1, 1, 2, 416)      # dilation 1


@pytest.mark.parametrize("is_3d", [False, True])
def test_pinned_convs_match_torch_autograd(is_3d):
    """on their first forward the drop-in modules pin their convolutions
    (_precision.pin_fp32_convs) -- same parameters and state dict, class Pinned*, whose autograd
    forward/backward are aten's convolution with TF32 off whoever calls backward.  The values and
    every gradient equal torch's own autograd through the plain modules (here on the CPU, where
    both are the same convolution), for the 2-D / 3-D convs and their transposed forms."""
    import copy

    from aanet_amd import _precision
    from aanet_amd.nets.feature import Conv2x
    torch.manual_seed(0)
    m = Conv2x(8, 4, deconv=True, is_3d=is_3d)
    ref = copy.deepcopy(m)
    ref.__dict__["_aanet_pinned"] = True  # the reference copy keeps plain torch modules
    for mod in ref.modules():
        mod.__dict__["_aanet_pinned"] = True
    shape = (2, 8, 3, 4, 5) if is_3d else (2, 8, 5, 6)
    x = torch.randn(shape, requires_grad=True)
    rem_shape = (2, 4, 5, 8, 10) if is_3d else (2, 4, 10, 12)
    rem = torch.randn(rem_shape, requires_grad=True)
    x2, rem2 = x.detach().clone().requires_grad_(), rem.detach().clone().requires_grad_()
    out, out2 = m(x, rem), ref(x2, rem2)
    pinned = {type(mod) for mod in m.modules() if isinstance(mod, (torch.nn.modules.conv._ConvNd))}
    assert pinned == ({_precision.PinnedConvTranspose3d, _precision.PinnedConv3d} if is_3d else
                      {_precision.PinnedConvTranspose2d, _precision.PinnedConv2d}), pinned
    assert all(type(mod).__module__.startswith("torch") for mod in ref.modules()
               if isinstance(mod, torch.nn.modules.conv._ConvNd))
    assert m.state_dict().keys() == ref.state_dict().keys()
    g = torch.randn(out.shape)
    out.backward(g)
    out2.backward(g)
    assert torch.allclose(out, out2, atol=1e-6)
    assert torch.allclose(x.grad, x2.grad, atol=1e-5) and torch.allclose(rem.grad, rem2.grad, atol=1e-5)
    for (n, p), (_, p2) in zip(m.named_parameters(), ref.named_parameters()):
        assert torch.allclose(p.grad, p2.grad, atol=1e-4, rtol=1e-5), n


@pytest.mark.parametrize("ci,co,h,w", [(8, 4, 5, 7), (3, 6, 1, 1), (16, 8, 4, 9)])
def test_deconv2x_phase_weight_is_the_transposed_conv(ci, co, h, w):
    """ops.deconv2x's decomposition on the CPU: the 2x2 pad-1 conv with the phase weight
    (deconv2x_phase_weight), its output [4c+2a+b][y+a][x+b] scattered to [c][2y+a][2x+b] (what
    aanet_deconv2x_assemble_f32 does), equals ConvTranspose2d(k=4, s=2, p=1) in fp64."""
    g = torch.Generator().manual_seed(ci * 100 + co)
    x = torch.randn(2, ci, h, w, generator=g, dtype=torch.float64)
    wt = torch.randn(ci, co, 4, 4, generator=g, dtype=torch.float64)
    scale = torch.rand(co, generator=g, dtype=torch.float64) + 0.5
    ref = torch.nn.functional.conv_transpose2d(x, wt * scale.view(1, -1, 1, 1), stride=2, padding=1)
    ph = torch.nn.functional.conv2d(x, ops.deconv2x_phase_weight(wt, scale), padding=1)
    assert ph.shape == (2, 4 * co, h + 1, w + 1)
    out = torch.empty_like(ref)
    for a in (0, 1):
        for b in (0, 1):
            out[:, :, a::2, b::2] = ph[:, 2 * a + b::4, a:a + h, b:b + w]
    assert torch.allclose(out, ref, rtol=0, atol=1e-12)


# ------------------------------------------------------- conv engine plan (aanet_conv_engine_plan)
SPLIT = _lib.CONV_WEIGHTS_SPLIT


def test_engine_plan_tile_width_threshold_without_a_gpu():
    """The engine takes 128-pixel tiles when N * ceil(P / 128) * groups * ncot >= 512, else 64
    (64 -> 64 3x3 s1 p1, NCHW input, split weights: no halo form): N = 4 at 113 x 145 is 516
    workgroups with one valid pixel in the last tile, N = 3 (387) stays on 64-pixel tiles, and
    N = 8 at 65 x 125 sits exactly on 512 with 61 valid pixels in the last."""
    plan = lambda n, h, w: ops.conv_engine_plan("conv", n, 64, h, w, 64, 3, 1, 1, layout=SPLIT)  # noqa: E731
    a = plan(4, 113, 145)
    assert (a.status, a.ptt, a.co_t, a.halo, a.prec, a.full, a.cfg) == (0, 128, 64, 0, 1, 1, 0)
    assert (a.last_tile_pixels, a.grid_x, a.grid_y) == (1, 4 * 129, 1)
    b = plan(3, 113, 145)
    assert (b.status, b.ptt, b.last_tile_pixels, b.grid_x) == (0, 64, 113 * 145 % 64, 3 * 257)
    c = plan(8, 65, 125)
    assert (c.status, c.ptt, c.last_tile_pixels, c.grid_x * c.grid_y) == (0, 128, 61, 512)
    # one workgroup fewer: 7 images are 448 workgroups of 128 pixels
    assert plan(7, 65, 125).ptt == 64
    # groups and output-channel tiles count towards the threshold: Co = 128 halves N
    d = ops.conv_engine_plan("conv", 2, 64, 113, 145, 128, 3, 1, 1, layout=SPLIT)
    assert (d.ptt, d.grid_x, d.grid_y) == (128, 2 * 129, 2)
    assert ops.conv_engine_plan("conv", 1, 64, 113, 145, 128, 3, 1, 1, layout=SPLIT).ptt == 64


def test_engine_plan_forms_that_always_take_128_pixel_tiles():
    """co_t = 16, 16-channel chunks (cfg 1) and every halo form run 128-pixel tiles at any size."""
    p = ops.conv_engine_plan("conv", 1, 5, 7, 9, 3, 3, 1, 1, packed=False)
    assert (p.status, p.co_t, p.ptt, p.full, p.prec, p.packed) == (0, 16, 128, 0, 0, 0)
    p = ops.conv_engine_plan("conv", 1, 32, 9, 26, 54, 3, 1, 2, 2, groups=2, layout=1)
    assert (p.status, p.co_t, p.ptt, p.full, p.cfg, p.prec, p.layout) == (0, 32, 128, 1, 1, 0, 1)
    for dil, layout, halo in ((1, 1, 1), (2, 1, 2), (1, 3, 1), (4, 3, 4), (8, 3, 4)):
        p = ops.conv_engine_plan("conv", 1, 64, 9, 26, 64, 3, 1, dil, dil, layout=layout | SPLIT)
        assert (p.status, p.halo, p.ptt, p.prec, p.layout) == (0, halo, 128, 1, layout), (dil, p)
    # 9 x 26 on 16 x 8 halo tiles: one ragged row, ten ragged columns
    p = ops.conv_engine_plan("conv", 1, 64, 9, 26, 64, 3, 1, 1, layout=1 | SPLIT)
    assert (p.last_tile_rows, p.last_tile_cols, p.last_tile_pixels, p.grid_x) == (1, 10, 10, 4)
    # the halo forms need the split contraction, NHWC input and stride 1
    assert ops.conv_engine_plan("conv", 1, 64, 9, 26, 64, 3, 1, 1, layout=1).halo == 0
    assert ops.conv_engine_plan("conv", 1, 64, 9, 26, 64, 3, 1, 1, layout=SPLIT).halo == 0
    assert ops.conv_engine_plan("conv", 1, 64, 9, 26, 64, 3, 2, 1, layout=1 | SPLIT).halo == 0
    assert ops.conv_engine_plan("conv", 1, 64, 9, 26, 64, 3, 1, 1,
                                layout=1 | SPLIT | _lib.CONV_EXACT_F32).halo == 0


def test_engine_plan_contraction_and_chunks():
    """C % 32 == 16 with a split pack and NCHW input: guarded (zero-padded) chunks on the split
    contraction (full 0, prec 1); the same on exact f32 or with a plain pack is 16-channel full
    chunks (cfg 1) in exact f32.  The DCN's chunk configurations; the tail's layouts."""
    for c in (48, 80):
        p = ops.conv_engine_plan("conv", 2, c, 24, 52, 64, 3, 1, 1, layout=SPLIT)
        assert (p.status, p.full, p.cfg, p.prec, p.layout) == (0, 0, 0, 1, 0), p
        p = ops.conv_engine_plan("conv", 2, c, 24, 52, 64, 3, 1, 1, layout=SPLIT | _lib.CONV_EXACT_F32)
        assert (p.status, p.full, p.cfg, p.prec, p.ptt) == (0, 1, 1, 0, 128), p
    p = ops.conv_engine_plan("dcn", 2, 64, 16, 52, 64, 3, 1, 2, 2, deformable_groups=2, layout=SPLIT)
    assert (p.status, p.full, p.cfg, p.prec, p.ptt) == (0, 1, 0, 1, 64)
    p = ops.conv_engine_plan("dcn", 2, 32, 16, 52, 32, 3, 1, 2, 2, deformable_groups=2, layout=SPLIT)
    assert (p.status, p.full, p.cfg, p.prec, p.co_t) == (0, 1, 2, 0, 32)
    p = ops.conv_engine_plan("dcn", 2, 64, 16, 52, 64, 3, 1, 2, 2, deformable_groups=2, packed=False)
    assert (p.status, p.full, p.prec, p.packed) == (0, 1, 0, 0)
    for layout in (0, 1):
        p = ops.conv_engine_plan("conv", 2, 64, 25, 36, 64, 3, 2, 1, co2=64, layout=layout | SPLIT)
        assert (p.status, p.tail, p.layout, p.prec, p.halo) == (0, 1, layout, 1, 0)
    # the tail's tile covers max(co, co2)
    assert ops.conv_engine_plan("conv", 2, 32, 9, 26, 16, 3, 1, 1, co2=32).co_t == 32


def test_engine_plan_refusals_match_the_launch_without_a_gpu():
    """What launch_fwd refuses comes back from the plan with the same status, and -- for the
    shapes an entry point can express -- from the entry point itself (dummy pointers: the
    refusal comes before any launch)."""
    import ctypes as C
    U, E = _lib.EUNSUPPORTED, -1
    plan = ops.conv_engine_plan
    assert plan("conv", 1, 64, 8, 8, 128, 3, 1, 1, co2=64).status == U        # tail with Co > 64
    assert plan("conv", 1, 64, 8, 8, 64, 3, 1, 1, co2=65).status == U         # ... or Co2 > 64
    assert plan("conv", 1, 64, 8, 8, 64, 3, 1, 1, co2=64, packed=False).status == U
    assert plan("conv", 1, 24, 8, 8, 32, 3, 1, 1, layout=1).status == U       # NHWC, 24 channels
    assert plan("conv", 1, 16, 8, 8, 16, 3, 1, 1, layout=1).status == U       # 16-ch chunks, co_t 16
    assert plan("conv", 1, 64, 8, 8, 54, 3, 1, 1, groups=2, layout=2).status == U   # Cog % 4
    assert plan("conv", 1, 64, 8, 8, 64, 3, 1, 1, co2=64, layout=2).status == U     # NHWC out + tail
    assert plan("conv", 1, 64, 8, 10, 64, 3, 1, 1, co2=64, csa=[(4, 5)]).status == U   # CSA, Wo % 4
    assert plan("conv", 1, 64, 8, 8, 64, 3, 1, 1, co2=64, csa=[(4, 4)]).status == 0
    assert plan("conv", 1, 64, 8, 8, 64, 3, 1, 1, co2=64, csa=[(3, 3)]).status == U    # not 2x / 4x
    assert plan("conv", 1, 64, 8, 8, 64, 3, 1, 1, co2=64, csa=[(4, 4), (2, 2), (1, 1)]).status == U
    assert plan("conv", 1, 64, 8, 8, 64, 3, 1, 1, csa=[(4, 4)]).status == U            # CSA, no tail
    assert plan("dcn", 1, 64, 8, 1, 64, 3, 1, 1, deformable_groups=2).status == U      # DCN, W < 2
    assert plan("dcn", 1, 64, 8, 2, 64, 3, 1, 1, deformable_groups=2).status == 0
    # the post stage has one form: HALO 1 tail (split, NHWC input, dil 1) with CSA, 64 -> 64
    post = dict(co2=64, csa=[(4, 4)], layout=1 | SPLIT)
    ok = plan("conv", 1, 64, 8, 8, 64, 3, 1, 1, post=1, **post)
    assert (ok.status, ok.post, ok.halo, ok.tail) == (0, 1, 1, 1)
    assert plan("conv", 1, 64, 8, 8, 64, 3, 1, 1, post=2, **post).status == U          # disp / skip
    assert plan("conv", 1, 64, 8, 8, 64, 3, 1, 2, 2, post=1, **post).status == U       # dil 2
    assert plan("conv", 1, 64, 8, 8, 64, 3, 1, 1, post=1, co2=64, csa=[(4, 4)], layout=1).status == U
    assert plan("conv", 1, 64, 8, 8, 64, 3, 1, 1, post=1, co2=64, layout=1 | SPLIT).status == U
    assert plan("dcn", 1, 64, 8, 8, 64, 3, 1, 1, deformable_groups=2, post=1, **post).status == U
    # invalid sizes
    assert plan("conv", 1, 64, 8, 8, 64, 3, 0, 1).status == E                 # stride 0
    assert plan("conv", 1, 63, 8, 8, 64, 3, 1, 1, groups=2).status == E
    assert plan("conv", 1, 64, 2, 8, 64, 5, 1, 0).status == E                 # no output rows
    assert plan("conv", 1, 64, 8, 8, 64, 3, 1, 1, layout=4).status == E
    assert plan("conv", 1, 64, 8, 8, 64, 3, 1, 1, layout=_lib.CONV_GENERIC_DCN).status == E
    assert plan("conv", 1, 1 << 16, 128, 128, 64, 1).status == U              # 2^31-byte planes
    # ... and the same from the entry points
    L = _lib.lib()
    p = C.c_void_p(16)
    fused = lambda *shape: L.aanet_conv2d_fused_f32(p, p, None, None, None, None, 0, 1, p, *shape, None)  # noqa: E731
    assert fused(1, 24, 8, 8, 32, 3, 3, 1, 1, 1, 1, 1) == U
    assert fused(1, 64, 8, 8, 54, 3, 3, 1, 1, 1, 2, 2) == U
    assert fused(1, 64, 8, 8, 64, 3, 3, 1, 1, 1, 1, 4) == E
    assert fused(1, 64, 8, 8, 64, 3, 3, 0, 1, 1, 1, 0) == E                   # stride 0: no SIGFPE
    pw = lambda co, co2, w, desc: L.aanet_conv2d_pw_f32(  # noqa: E731
        p, p, None, None, None, 0, p, None, None, 0, co2, p, 1, 64, 8, w, co, 3, 3, 1, 1, 1, desc, 0, None)
    assert pw(128, 64, 8, None) == U
    d = _lib.CsaEpilogue()
    d.out, d.num_up = 16, 1
    d.up[0], d.up_h[0], d.up_w[0] = 16, 4, 5
    assert pw(64, 64, 10, C.byref(d)) == U
    assert L.aanet_mdcn_fwd_f32(p, p, p, p, None, p, 1, 64, 8, 1, 64, 3, 3, 1, 1, 1, 1, 2, None) == U


def test_engine_plan_descriptor_sizes_are_checked():
    import ctypes as C
    L = _lib.lib()
    q, pl = _lib.ConvPlanQuery(), _lib.ConvPlan()
    assert q.struct_size == C.sizeof(q) and pl.struct_size == C.sizeof(pl)
    assert L.aanet_conv_engine_plan(None, C.byref(pl)) == -1
    q.struct_size -= 4
    assert L.aanet_conv_engine_plan(C.byref(q), C.byref(pl)) == _lib.EABI
    q.struct_size += 4
    pl.struct_size = 8
    assert L.aanet_conv_engine_plan(C.byref(q), C.byref(pl)) == _lib.EABI
    with pytest.raises(_lib.AanetError):
        _lib.call("aanet_conv_engine_plan", C.byref(q), C.byref(pl))


def test_nhwc_assembly_refuses_more_than_496_channels_without_a_gpu():
    """aanet_concat_nhwc_f32 / aanet_deconv2x_assemble_nhwc_f32 stage every channel of 64 (up to
    252 channels) or 32 (up to 496) output columns in 64 KiB of LDS: 497 channels come back as
    AANET_EUNSUPPORTED from the host, before any launch (dummy pointers)."""
    import ctypes as C
    L = _lib.lib()
    p = C.c_void_p(16)
    assert 496 * 33 * 4 <= 64 * 1024 < 497 * 33 * 4 and 252 * 65 * 4 <= 64 * 1024 < 253 * 65 * 4
    assert L.aanet_concat_nhwc_f32(p, p, p, 2, 200, 297, 4, 10, None) == _lib.EUNSUPPORTED
    assert L.aanet_deconv2x_assemble_nhwc_f32(p, p, p, 2, 249, 248, 4, 10, None) == _lib.EUNSUPPORTED
    assert L.aanet_concat_nhwc_f32(p, p, p, 2, 200, 296, 5, 10, None) == _lib.EUNSUPPORTED  # odd h
