"""Case table of the feature- and refinement-stage sweep (helper, no tests).

tests/hotpath_sweep.py holds the adaptive-aggregation dispatch layer to a table; this one does
the same for the other two Python layers that pick HIP kernels in the eval forward: the feature
stage (nets/feature.py, nets/resnet.py and the parts of nets/_fuse.py / nets/deform.py they call)
and the refinement stage (nets/refinement.py).  A row is one whole-stage run:

    Row(id, stage, kwargs, B, image, extra, seed, expect)

  stage    class name in aanet_amd.nets.{feature,resnet,refinement}
  kwargs   constructor arguments
  B        batch
  image    (H, W) of the input image (of the finest feature map for the two pyramid classes)
  extra    the other input sizes: None (feature extractors), the coarser pyramid levels
           (FeaturePyramidNetwork), the low-resolution disparity's (h, w) (refinement)
  seed     of fill_synthetic(module, seed) and of every input generator
  expect   the value of every dispatch predicate the stage consults on the row's shapes, as
           LITERALS: a dispatch change shows up as a diff of this table (`census` says what each
           column is; tests/test_stage_sweep_cpu.py evaluates them on the CPU)

The columns are not restated predicates: `fused_on_cpu` runs the stage's own eval fast path on
CPU tensors, with the device test of `use_fused` lifted and every `ops` launch replaced by a
torch / C-oracle computation of the same operation that checks the arguments as the real wrapper
does, and records what was consulted and what would have been launched.  Because the stand-ins
compute, the same run also checks the Python layer's arithmetic (BN folding, phase weights,
residual routing, activations) against the reference-order module in float64, without a GPU.

`reference64` is the float64 (or CPU float32) reference-order twin of a stage;
`expected_launches` turns a row's columns into the C entry points the fused run must and must
not call; tests/test_gpu_stage_sweep.py holds the device to both.
"""
import collections
import contextlib
import copy
import functools

import numpy as np
import torch
import torch.nn.functional as F

Row = collections.namedtuple("Row", "id stage kwargs B image extra seed expect")

# The entry points whose presence the dispatch predicates decide.
CENSUS_ENTRIES = ("aanet_conv3x3s2_f32", "aanet_deconv2x_assemble_f32",
                  "aanet_deconv2x_assemble_nhwc_f32", "aanet_concat_nhwc_f32",
                  "aanet_refine_stem_f32", "aanet_disp_warp_f32",
                  "aanet_conv3x3_grouped_nhwc_f32", "aanet_mdcn_fwd_fused_f32",
                  "aanet_conv2d_pw_f32", "aanet_conv2d_fused_f32")

# Entries that cannot be both launched in one row and absent from another ({entry: reason}).
# aanet_resize_bilinear_f32 is not listed at all: no stage calls ops.resize_bilinear (the
# refinement's upsampling and PSMNet's SPP go through F.interpolate).
ENTRY_NOT_REQUIRED = {
    "aanet_conv2d_fused_f32": "every stage has a plain conv on the engine: launched in every row",
    "aanet_conv2d_pw_f32": "the tail kernel needs width <= 64 and <= 64 outputs; every bottleneck "
                           "of AANetFeature expands x4 to >= 128: launched in no row",
    "aanet_conv3x3_grouped_nhwc_f32": "reached only by AANetFeature layer3's offset convs (two "
                                      "groups of 64 channels), which the kernel refuses before "
                                      "any launch: returns in no row (the hot-path sweep and "
                                      "tests/test_gpu_conv_g3.py launch it)",
    "aanet_deconv2x_assemble_f32": "the NCHW assembly runs when a Conv2x deconv misses the "
                                   "one-pass concat (rem not twice x) or feeds a DCN conv2; the "
                                   "hourglasses' legal sizes (multiples of 48 / 16) halve exactly "
                                   "and their deconv Conv2x all have plain conv2: launched in no "
                                   "row (tests/test_gpu_deconv.py covers the op)",
}

# Predicate columns that cannot take both values inside the table's legal range.
NOT_REQUIRED = {
    "aten_convs": "every conv of both stages has a HIP route in eval: 0 in every row",
    "g3_launch": "the only offset convs with a packing that the stages reach with NHWC input are "
                 "AANetFeature layer3's, which conv_g3 refuses: false wherever consulted",
    "stem_fused": "_stem_fused refuses only images that are not 3-channel or a stem whose convs "
                  "are not the constructor's: true wherever the stage has a stem",
    "dilated_nhwc": "_DilatedStack leaves the channels-last route only for blocks that are not "
                    "the constructor's (a downsample, another norm layer): true in every row",
    "out_format": "channels-last tensors stay inside the stages (laterals, the hourglass's last "
                  "block, the dilated stack): every returned tensor is NCHW-contiguous",
}

T, F_ = True, False


def _x(halo="", s2_conv="", deconv2x="", offset_pack="", g3_launch="", routes="", stem_fused=None,
       resize_skipped=None, dilated_nhwc=None, fpn_nhwc=None, stem_nhwc=None,
       out_format=("nchw",), aten_convs=0):
    return dict(halo=halo, s2_conv=s2_conv, deconv2x=deconv2x, offset_pack=offset_pack,
                g3_launch=g3_launch, routes=routes, stem_fused=stem_fused, resize_skipped=resize_skipped,
                dilated_nhwc=dilated_nhwc, fpn_nhwc=fpn_nhwc, stem_nhwc=stem_nhwc,
                out_format=out_format, aten_convs=aten_convs)


# expect columns (strings: one letter per consultation, in call order):
#   halo         halo_input_ok: AANetFeature one per plain bottleneck (conv2 of layer1 x3, layer2
#                x4[, layer3 x6]); hourglass one per Conv2x whose earlier tests pass; FPN one per
#                output conv (all() stops at the first F)
#   s2_conv      s2_conv_ok in conv_bn_act_s2: bottleneck conv2 past the tail kernel, BasicConv
#   deconv2x     deconv2x_ok per Conv2x (T the 4x4 transposed conv1, F a plain conv1)
#   offset_pack  offset_conv_pack finds a packing, per offset conv reached with NHWC input
#   g3_launch    per ops.conv3x3_grouped_nhwc call: T the kernel has the instance, F it answers
#                "unsupported" and offset_conv_eval falls back to the engine
#   routes       per Conv2x: D deconv + concat in one assembly pass, channels-last out; d the same
#                NCHW out; N ops.concat_nhwc; C torch.cat
#   stem_fused / resize_skipped / dilated_nhwc   refinement: _stem_fused; _upsampled_disp returned
#                its input; _DilatedStack ran channels-last
#   fpn_nhwc     FeaturePyramidNetwork wrote its laterals channels-last
#   stem_nhwc    GANetFeature took the NHWC-stem branch
#   out_format   memory format of each returned tensor
#   aten_convs   aten::convolution calls of the fused run (0: a HIP route for every conv)
# layer3's offset convs (128 -> 54, two groups of 64 channels) have a packing, but conv_g3 has no
# instance for two K chunks per group with two groups: refused, the engine runs them
_AA_MD = dict(halo="TTTFTTT", s2_conv="FFFTFFF", offset_pack="TTTTT", g3_launch="FFFFF")
_AA_PLAIN = dict(halo="TTTFTTTFTTTTT", s2_conv="FFFTFFFFFFFFF")
_GA_D = "TTTTFFFFTTTT"
# BasicConv consults s2_conv_ok for every 4-D plain conv, the stride-1 ones included.  T: conv1a
# and conv1b's conv1 (32 -> 48), and when they are plain conv3a and conv3b's conv1 (64 -> 96);
# conv2a / conv2b (48 inputs) and conv4a / conv4b (128 outputs) fall to the engine
_GA_S2 = "FFFTFTFFFFFTFFFTFFFFFFF"
_GA_MD_S2 = "FTFFFFFTFFFTFFFFF"
_HG_S2 = "TFFFFFTFFFTFFFF"

def _rows():
    aa = lambda md: dict(feature_mdconv=md)  # noqa: E731
    fpn = lambda cin, co, n: dict(in_channels=cin, out_channels=co, num_levels=n)  # noqa: E731
    n3 = ("nchw",) * 3
    ga = lambda routes, halo, **k: _x(halo=halo, s2_conv=k.pop("s2", _GA_S2),  # noqa: E731
                                      deconv2x=_GA_D, routes=routes, **k)
    return [
        # ---- AANetFeature: 7x7 stride-3 stem, layer1 at H/3, layer2 / layer3 ceil-halved
        Row("aa_md_48x96", "AANetFeature", aa(T), 2, (48, 96), None, 101, _x(**_AA_MD, out_format=n3)),
        Row("aa_md_37x61", "AANetFeature", aa(T), 1, (37, 61), None, 102, _x(**_AA_MD, out_format=n3)),
        Row("aa_md_25x400", "AANetFeature", aa(T), 1, (25, 400), None, 103, _x(**_AA_MD, out_format=n3)),
        Row("aa_md_7x10", "AANetFeature", aa(T), 3, (7, 10), None, 104,
            # layer3 runs at 1x1: a channels-last 1x1 map is also NCHW-contiguous, is_nhwc is false
            # and the offset convs go to the engine without asking for a packing
            _x(**{**_AA_MD, "offset_pack": "", "g3_launch": ""}, out_format=n3)),
        Row("aa_48x96", "AANetFeature", aa(F_), 1, (48, 96), None, 105, _x(**_AA_PLAIN, out_format=n3)),
        Row("aa_37x61", "AANetFeature", aa(F_), 3, (37, 61), None, 106, _x(**_AA_PLAIN, out_format=n3)),
        Row("aa_25x400", "AANetFeature", aa(F_), 2, (25, 400), None, 107, _x(**_AA_PLAIN, out_format=n3)),
        Row("aa_7x10", "AANetFeature", aa(F_), 1, (7, 10), None, 108, _x(**_AA_PLAIN, out_format=n3)),
        # ---- GANetFeature: H/3, then four exact halvings; the bottom level decides conv4b
        Row("ga_48x96", "GANetFeature", aa(F_), 1, (48, 96), None, 111,
            ga("DDDDNNNCDDDD", "TTTTTTTTTTT", stem_nhwc=F_)),
        Row("ga_96x48", "GANetFeature", aa(F_), 1, (96, 48), None, 112,
            ga("DDDDNNNCDDDD", "TTTTTTTTTTT", stem_nhwc=F_)),
        Row("ga_48x240", "GANetFeature", aa(F_), 1, (48, 240), None, 113,
            ga("DDDDNNNCDDDD", "TTTTTTTTTTT", stem_nhwc=F_)),
        Row("ga_96x144", "GANetFeature", aa(F_), 2, (96, 144), None, 114,
            ga("DDDDNNNCDDDD", "TTTTTTTTTTT", stem_nhwc=F_)),
        Row("ga_96x96", "GANetFeature", aa(F_), 1, (96, 96), None, 117,   # 2x2 bottom: conv4b on N
            ga("DDDDNNNNDDDD", "TTTTTTTTTTTT", stem_nhwc=F_)),
        Row("ga_md_48x96", "GANetFeature", aa(T), 2, (48, 96), None, 115,
            ga("DDDDNNCCDDDD", "TTTTTTTTTT", stem_nhwc=T, s2=_GA_MD_S2, offset_pack="F")),
        Row("ga_md_96x144", "GANetFeature", aa(T), 1, (96, 144), None, 116,
            ga("DDDDNNCCDDDD", "TTTTTTTTTT", stem_nhwc=T, s2=_GA_MD_S2, offset_pack="F")),
        # ---- StereoNetFeature: 5x5 stride-2 stem convs, ceil-halved
        Row("sn_d3_75x133", "StereoNetFeature", dict(num_downsample=3), 2, (75, 133), None, 121, _x()),
        Row("sn_d3_8x8", "StereoNetFeature", dict(num_downsample=3), 1, (8, 8), None, 122, _x()),
        Row("sn_d1_21x30", "StereoNetFeature", dict(num_downsample=1), 1, (21, 30), None, 123, _x()),
        # ---- PSMNetFeature: the 64x64 average pool needs a 1/4 map of at least 64 x 64
        Row("psm_256x272", "PSMNetFeature", {}, 1, (256, 272), None, 131, _x()),
        Row("psm_253x300", "PSMNetFeature", {}, 1, (253, 300), None, 132, _x()),
        Row("gc_37x90", "GCNetFeature", {}, 1, (37, 90), None, 141, _x()),
        Row("gc_64x64", "GCNetFeature", {}, 2, (64, 64), None, 142, _x()),
        # ---- FeaturePyrmaid(32): two 3x3 stride-2 + 1x1 levels from one map
        Row("pyr_16x40", "FeaturePyrmaid", dict(in_channel=32), 2, (16, 40), None, 151, _x(out_format=n3)),
        Row("pyr_13x37", "FeaturePyrmaid", dict(in_channel=32), 1, (13, 37), None, 152, _x(out_format=n3)),
        Row("pyr_5x9", "FeaturePyrmaid", dict(in_channel=32), 1, (5, 9), None, 153, _x(out_format=n3)),
        # ---- FeaturePyramidNetwork at the production width, and at 48 (laterals stay NCHW)
        Row("fpn_12x20", "FeaturePyramidNetwork", fpn([128, 256, 512], 128, 3), 2, (12, 20),
            [(6, 10), (3, 5)], 161, _x(halo="TTT", fpn_nhwc=T, out_format=n3)),
        Row("fpn_16x42_two", "FeaturePyramidNetwork", fpn([128, 256], 128, 2), 1, (16, 42),
            [(8, 21)], 162, _x(halo="TT", fpn_nhwc=T, out_format=n3[:2])),
        Row("fpn_12x20_co48", "FeaturePyramidNetwork", fpn([128, 256, 512], 48, 3), 1, (12, 20),
            [(6, 10), (3, 5)], 163, _x(halo="F", fpn_nhwc=F_, out_format=n3)),
        # ---- refinement: image size, low-resolution disparity size
        Row("snr_37x61", "StereoNetRefinement", {}, 2, (37, 61), (5, 8), 171,
            _x(resize_skipped=F_, dilated_nhwc=T)),
        Row("snr_24x40_same", "StereoNetRefinement", {}, 1, (24, 40), (24, 40), 172,
            _x(resize_skipped=F_, dilated_nhwc=T)),
        Row("dr_37x61", "StereoDRNetRefinement", {}, 1, (37, 61), (13, 21), 181,
            _x(stem_fused=T, resize_skipped=F_, dilated_nhwc=T)),
        Row("dr_13x300", "StereoDRNetRefinement", {}, 2, (13, 300), (5, 100), 182,
            _x(stem_fused=T, resize_skipped=F_, dilated_nhwc=T)),
        Row("dr_24x40_same", "StereoDRNetRefinement", {}, 1, (24, 40), (24, 40), 183,
            _x(stem_fused=T, resize_skipped=T, dilated_nhwc=T)),
        Row("hg_16x32", "HourglassRefinement", {}, 1, (16, 32), (6, 11), 191,
            ga("DDDDNNCCDDDD", "TTTTTTTTTT", s2=_HG_S2, offset_pack="F", stem_fused=T,
               resize_skipped=F_)),
        Row("hg_48x80", "HourglassRefinement", {}, 2, (48, 80), (16, 27), 192,
            ga("DDDDNNCCDDDD", "TTTTTTTTTT", s2=_HG_S2, offset_pack="F", stem_fused=T,
               resize_skipped=F_)),
        Row("hg_32x112_same", "HourglassRefinement", {}, 1, (32, 112), (32, 112), 193,
            ga("DDDDNNCCDDDD", "TTTTTTTTTT", s2=_HG_S2, offset_pack="F", stem_fused=T,
               resize_skipped=T)),
    ]


ROWS = _rows()
BY_ID = {r.id: r for r in ROWS}
assert len(BY_ID) == len(ROWS)

REFINEMENT = ("StereoNetRefinement", "StereoDRNetRefinement", "HourglassRefinement")


def is_refinement(row):
    return row.stage in REFINEMENT


def has_dcn(row):
    return row.stage == "HourglassRefinement" or bool(row.kwargs.get("feature_mdconv"))


def has_warp(row):
    return row.stage in ("StereoDRNetRefinement", "HourglassRefinement")


def build(row):
    """The row's module in eval mode on the CPU (float32) with its synthetic weights."""
    from aanet_amd.nets import feature, refinement, resnet
    from tests.golden_io import fill_synthetic
    cls = next(getattr(mod, row.stage) for mod in (feature, resnet, refinement)
               if hasattr(mod, row.stage))
    m = cls(**row.kwargs)
    fill_synthetic(m, row.seed)
    return m.eval()


def low_disparity(B, size, seed):
    """[B, h, w] low-resolution disparity for the refinement rows: smooth and positive in
    [0, w/4] low-resolution pixels (so [0, W/4] at the image size), plus noise, with a block of
    whole numbers.  Column 0 is > 0, so the warp reaches the left border clip; the block gives
    integer sampling positions where the stage does not resize.  Its own generator stream (seed
    base 9000): no fixture depends on it."""
    h, w = size
    g = torch.Generator().manual_seed(9000 + seed)
    ys = torch.linspace(0, 1, h).view(1, h, 1)
    xs = torch.linspace(0, 1, w).view(1, 1, w)
    phase = torch.rand(B, 1, 1, generator=g) * 6.28
    smooth = 0.5 + 0.25 * torch.sin(3.0 * xs + phase) + 0.2 * torch.cos(2.0 * ys + phase)
    d = (w / 4.0) * (smooth + 0.04 * torch.randn(B, h, w, generator=g)).clamp(0.02, 1.0)
    d[:, h // 3: h // 3 + max(1, h // 4), w // 2: w // 2 + max(1, w // 4)] = float(max(1, w // 8))
    return d.contiguous()


def inputs(row):
    """The positional arguments of the row's forward, float32 CPU tensors."""
    from tests.golden_io import synthetic_pair, synthetic_pyramid_sizes
    H, W = row.image
    if row.stage == "FeaturePyrmaid":
        return (synthetic_pyramid_sizes(row.B, row.kwargs["in_channel"], [row.image], row.seed)[0][0],)
    if row.stage == "FeaturePyramidNetwork":
        sizes = [row.image] + list(row.extra)
        return ([synthetic_pyramid_sizes(row.B, c, [s], row.seed + 17 * i)[0][0]
                 for i, (c, s) in enumerate(zip(row.kwargs["in_channels"], sizes))],)
    left, right = synthetic_pair(row.B, H, W, row.seed)
    if is_refinement(row):
        return low_disparity(row.B, row.extra, row.seed), left, right
    return (left,)


def cast(args, dtype=None, device=None):
    def one(a):
        return [one(v) for v in a] if isinstance(a, (list, tuple)) else a.to(device=device, dtype=dtype)
    return tuple(one(a) for a in args)


def levels(out):
    """A stage's result as a list of tensors (one level for the single-output stages)."""
    return list(out) if isinstance(out, (list, tuple)) else [out]


# ------------------------------------------------------------------ the reference twin ----
def disp_warp_reference(img, disp):
    """The reference warp formula in img's dtype with torch CPU ops: pixel grid minus the
    disparity along x, normalised to [-1, 1], grid_sample (bilinear, border padding,
    align_corners=True); the valid mask from a zero-padded sample of ones.  -> (warped, valid)."""
    B, _, H, W = img.shape
    xs = torch.arange(W, dtype=img.dtype).view(1, 1, W) - disp[:, 0]
    ys = torch.arange(H, dtype=img.dtype).view(1, H, 1).expand(B, H, W)
    grid = torch.stack((2 * (xs / (W - 1)) - 1, 2 * (ys / (H - 1)) - 1), dim=-1)
    warped = F.grid_sample(img, grid, mode="bilinear", padding_mode="border", align_corners=True)
    valid = F.grid_sample(torch.ones_like(img), grid, mode="bilinear", padding_mode="zeros",
                          align_corners=True)
    return warped, (valid >= 0.9999).to(img.dtype)


def _oracle_dcn_forward(dc, taps):
    """forward(x, offset, mask) of a ModulatedDeformConv on the C oracle, in x's dtype."""
    from oracle.aggregation import OracleMDCN
    from aanet_amd.nets._fuse import _int

    def forward(x, offset, mask):
        assert dc.groups == 1 and _int(dc.padding) == _int(dc.dilation)
        x, offset, mask = x.contiguous(), offset.contiguous(), mask.contiguous()
        taps.append((dc, x, offset, mask))
        return OracleMDCN.apply(x, offset, mask, dc.weight.detach(),
                                None if dc.bias is None else dc.bias.detach(),
                                _int(dc.dilation), dc.deformable_groups, _int(dc.stride))
    return forward


def reference64(module, dtype=torch.float64):
    """A deep copy of `module` on the CPU in `dtype` that runs the reference op order:
    `aanet_fuse` off on every submodule, every ModulatedDeformConv on the C oracle
    (oracle.mdcn_forward in that dtype, the module's own stride), the refinement's warp on
    disp_warp_reference.  `twin.dcn_taps` collects (deform_conv module, x, offset, mask) of every
    DCN call.  dtype=torch.float32 gives the CPU float32 reference-order run."""
    from aanet_amd.nets import refinement
    from aanet_amd.nets.deform_conv import ModulatedDeformConv
    twin = copy.deepcopy(module).cpu().to(dtype).eval()
    twin.dcn_taps = []
    for m in twin.modules():
        m.aanet_fuse = False
        m.__dict__.pop("_aanet_fold", None)
        if isinstance(m, ModulatedDeformConv):
            m.forward = _oracle_dcn_forward(m, twin.dcn_taps)
    if isinstance(twin, refinement._WarpErrorStem):
        inner = twin.forward

        def forward(*args, **kwargs):
            real = refinement.disp_warp
            refinement.disp_warp = disp_warp_reference
            try:
                return inner(*args, **kwargs)
            finally:
                refinement.disp_warp = real
        twin.forward = forward
    return twin


@functools.lru_cache(maxsize=None)
def reference(row_id):
    """{"ref64", "ref32": the twin's levels in float64 / CPU float32, as float64 numpy arrays}:
    computed once and shared (callers leave it unchanged)."""
    row = BY_ID[row_id]
    m, x = build(row), inputs(row)
    out = {}
    with torch.no_grad():
        for tag, dtype in (("ref64", torch.float64), ("ref32", torch.float32)):
            res = reference64(m, dtype)(*cast(x, dtype))
            assert all(t.dtype == dtype for t in levels(res))
            out[tag] = [t.numpy().astype(np.float64) for t in levels(res)]
    return out


def errors(got, ref):
    """(normwise, max elementwise relative to max|ref|, max|ref|), each at its worst level."""
    norm = max(float(np.linalg.norm(a - b) / np.linalg.norm(b)) for a, b in zip(got, ref))
    emax = max(float(np.abs(a - b).max() / np.abs(b).max()) for a, b in zip(got, ref))
    return norm, emax


def level_errors(got, ref):
    """Per level: (norm of the difference / norm of ref, max |difference|, max |ref|)."""
    return [(float(np.linalg.norm(a - b) / np.linalg.norm(b)), float(np.abs(a - b).max()),
             float(np.abs(b).max())) for a, b in zip(got, ref)]


# ------------------------------------------------------------------ fused path on the CPU -
class _OnDevice:
    """Stand-in for a tensor on the GPU: dense_grouped_ok reads only this."""
    is_cuda = True


def _act(y, act):
    if act in (None, 0):
        return y
    if act in ("relu", 1):
        return F.relu(y)
    assert act in ("leaky", 2), act
    return F.leaky_relu(y, 0.2)


def _check_layout(nhwc_ok, *tensors):
    """require_gpu's layout test: contiguous, or channels-last at the positions in nhwc_ok."""
    from aanet_amd._lib import is_nhwc
    for i, t in enumerate(tensors):
        if t is not None and not (t.is_contiguous() or (i in nhwc_ok and is_nhwc(t))):
            raise ValueError(f"arg{i} must be contiguous")


def has_split_pack(co, cg, k, g):
    from aanet_amd import _lib
    return _lib.lib().aanet_conv_weight_pack_split_bytes(co, cg, k, k, g) > 0


class Trace:
    """What a fused_on_cpu run consulted and would have launched."""

    def __init__(self):
        self.pred = collections.defaultdict(str)   # predicate column -> "TF..." in call order
        self.launches = []                         # C entry names, in call order
        self.engine = []                           # arguments of every engine conv (see _engine)
        self.routes = ""                           # per Conv2x.forward call
        self.aten_convs = 0
        self.resize_skipped = None
        self.deconv_rem = []                       # per ops.deconv2x call: rem given
        self._mine = 0

    @contextlib.contextmanager
    def own(self):
        """Around a stand-in's own torch ops: they are not the stage's aten convolutions."""
        self._mine += 1
        try:
            yield
        finally:
            self._mine -= 1

    def note(self, column, value):
        self.pred[column] += "T" if value else "F"

    def _engine(self, x, wshape, stride, padding, dilation, groups, out_nhwc, via):
        from aanet_amd._lib import is_nhwc
        N, C, H, W = x.shape
        co, cg, k, _ = wshape
        self.engine.append(dict(N=N, C=C, H=H, W=W, Co=co, k=k, s=stride, p=padding, d=dilation,
                                g=groups, layout=int(is_nhwc(x)) | 2 * int(bool(out_nhwc)),
                                split=has_split_pack(co, cg, k, groups), via=via))


def _patch_predicates(t, patch):
    """Wrap the dispatch predicates the two stages consult so that each call's answer lands in
    t.pred (and _upsampled_disp's skipped resize in t.resize_skipped); `patch(obj, name, value)`
    installs and remembers a replacement."""
    from aanet_amd.nets import _fuse, deform, feature, refinement

    def recorded(column, fn, truth=bool):
        def wrapper(*a, **k):
            r = fn(*a, **k)
            t.note(column, truth(r))
            return r
        return wrapper

    real_upsampled = refinement._upsampled_disp

    def upsampled_disp(low_disp, img, always_resize=False):
        out = real_upsampled(low_disp, img, always_resize)
        t.resize_skipped = out.data_ptr() == low_disp.data_ptr() and \
            tuple(out.shape[-2:]) == tuple(low_disp.shape[-2:])
        return out

    for mod in (feature, deform):
        patch(mod, "halo_input_ok", recorded("halo", _fuse.halo_input_ok))
    patch(_fuse, "s2_conv_ok", recorded("s2_conv", _fuse.s2_conv_ok))
    patch(feature, "deconv2x_ok", recorded("deconv2x", _fuse.deconv2x_ok))
    patch(_fuse, "offset_conv_pack",
          recorded("offset_pack", _fuse.offset_conv_pack, lambda r: r is not None))
    patch(refinement, "_upsampled_disp", upsampled_disp)


@contextlib.contextmanager
def recorded_predicates():
    """The predicate recording of fused_on_cpu alone, around a run on the device -> Trace (its
    pred and resize_skipped; nothing else is replaced)."""
    t, saved = Trace(), []

    def patch(obj, name, value):
        saved.append((obj, name, getattr(obj, name)))
        setattr(obj, name, value)

    _patch_predicates(t, patch)
    try:
        yield t
    finally:
        for obj, name, value in reversed(saved):
            setattr(obj, name, value)


@contextlib.contextmanager
def fused_on_cpu():
    """Run eval fast paths on CPU tensors -> Trace.  use_fused keeps its eval / no-grad /
    aanet_fuse tests and drops the device one; every ops launch the two stages reach is replaced
    by a stand-in that applies the real wrapper's argument checks, computes the operation with
    torch CPU ops (the DCN with the C oracle) in the input's dtype and records the entry point;
    the device packers return the weight itself where the real one has a packing."""
    from aanet_amd import _lib, ops
    from aanet_amd.nets import _fuse, deform, feature, refinement, resnet, warp
    from aanet_amd.nets._fuse import _int
    from oracle import oracle
    t = Trace()
    saved = []

    def patch(obj, name, value):
        saved.append((obj, name, getattr(obj, name)))
        setattr(obj, name, value)

    def use_fused(module, x):
        return (not module.training) and not torch.is_grad_enabled() and \
            getattr(module, "aanet_fuse", True)

    def conv2d_fused(x, weight, bias=None, stride=1, padding=0, dilation=1, groups=1, act=None,
                     residual=None, post_scale=None, post_shift=None, packed_weight=None,
                     out_nhwc=False, out=None, via="conv2d_fused"):
        _check_layout((0, 3) if out_nhwc else (0,), x, weight, bias, residual)
        with t.own():
            y = F.conv2d(x, weight, bias, stride, padding, dilation, groups)
            if residual is not None and tuple(residual.shape) != tuple(y.shape):
                raise ValueError("residual shape must match the output")
            if residual is not None and out_nhwc and not (_lib.is_nhwc(residual) or y.shape[1] == 1):
                raise ValueError("residual must be channels_last when out_nhwc=True")
            if post_scale is not None:
                y = y * post_scale.view(1, -1, 1, 1) + post_shift.view(1, -1, 1, 1)
            if residual is not None:
                y = y + residual
            y = _act(y, act)
        t._engine(x, weight.shape, stride, padding, dilation, groups, out_nhwc, via)
        t.launches.append("aanet_conv2d_fused_f32")
        return y.contiguous(memory_format=torch.channels_last) if out_nhwc else y.contiguous()

    def deconv2x(x, phase_weight, bias=None, act=None, packed_weight=None, rem=None,
                 out_nhwc=False):
        _check_layout((), x, phase_weight, bias, None, rem)
        N, C, H, W = x.shape
        co = phase_weight.shape[0] // 4
        t.deconv_rem.append(rem is not None)
        ph = conv2d_fused(x.contiguous(), phase_weight, bias, 1, 1, 1, 1, act, via="deconv2x")
        if rem is not None and tuple(rem.shape[0:1]) + tuple(rem.shape[2:]) != (N, 2 * H, 2 * W):
            raise ValueError("deconv2x: rem does not match the output")
        out = x.new_empty((N, co, 2 * H, 2 * W))
        for a in (0, 1):       # output (2y + a, 2x + b) of channel c is phase channel
            for b in (0, 1):   # 4c + 2a + b at (y + a, x + b)   (csrc/deconv.hip)
                out[:, :, a::2, b::2] = ph[:, 2 * a + b::4, a:a + H, b:b + W]
        if rem is not None:
            out = torch.cat((out, rem), 1)
        t.launches.append("aanet_deconv2x_assemble_nhwc_f32" if out_nhwc
                          else "aanet_deconv2x_assemble_f32")
        return out.contiguous(memory_format=torch.channels_last) if out_nhwc else out.contiguous()

    def concat_nhwc(a, b):
        if b.shape[0] != a.shape[0] or tuple(b.shape[2:]) != tuple(a.shape[2:]):
            raise ValueError("concat_nhwc: the tensors do not concatenate")
        if a.shape[2] % 2 or a.shape[3] % 2:  # what aanet_concat_nhwc_f32 answers
            raise _lib.AanetError("aanet_concat_nhwc_f32 failed: unsupported", _lib.EUNSUPPORTED)
        t.launches.append("aanet_concat_nhwc_f32")
        return torch.cat((a, b), 1).contiguous(memory_format=torch.channels_last)

    def refine_stem(warped, left, disp, w1, b1, w2, b2, act="leaky"):
        N, _, H, W = left.shape
        if tuple(warped.shape) != (N, 3, H, W) or tuple(disp.shape) != (N, 1, H, W) or \
                tuple(w1.shape) != (16, 6, 3, 3) or tuple(w2.shape) != (16, 1, 3, 3):
            raise ValueError("refine_stem: unexpected shapes")
        with t.own():
            y = torch.cat((_act(F.conv2d(torch.cat((warped - left, left), 1), w1, b1, 1, 1), act),
                           _act(F.conv2d(disp, w2, b2, 1, 1), act)), 1)
        t.launches.append("aanet_refine_stem_f32")
        return y.contiguous(memory_format=torch.channels_last)

    def disp_warp(img, disp, with_mask=True):
        _check_layout((), img, disp)
        if tuple(disp.shape) != (img.shape[0], 1) + tuple(img.shape[2:]):
            raise ValueError("disp must be [B, 1, H, W]")
        t.launches.append("aanet_disp_warp_f32")
        warped, valid = disp_warp_reference(img, disp)
        return warped, (valid if with_mask else None)

    def pack_conv3x3s2(weight):
        co, c, kh, kw = weight.shape
        return None if (kh, kw) != (3, 3) or co % 16 or co > 96 or c % 32 else weight

    def conv3x3_s2(x, wsplit, bias, co, co_a, act_a=None, act_b=None, x2=None, identity=None,
                   up=None):
        assert x2 is None and identity is None and up is None and wsplit.shape[0] == co
        _check_layout((), x, bias)
        with t.own():
            y = F.conv2d(x, wsplit, bias, 2, 1)
        t.launches.append("aanet_conv3x3s2_f32")
        return (_act(y[:, :co_a], act_a).contiguous() if co_a > 0 else None,
                _act(y[:, co_a:], act_b).contiguous() if co_a < co else None)

    def pack_conv3x3_grouped(weight, groups):
        co, cg, kh, kw = weight.shape
        if (kh, kw) != (3, 3) or \
                not _lib.lib().aanet_conv3x3_grouped_pack_bytes(co, cg * groups, groups):
            return None
        return weight

    def conv3x3_grouped_nhwc(x, wsplit, bias, co, groups, dilation):
        _check_layout((0,), x, bias)
        if not _lib.is_nhwc(x):
            raise ValueError("conv3x3_grouped_nhwc: x must be channels-last")
        # the instances aanet_conv3x3_grouped_nhwc_f32 has (csrc/conv_g3.hip): (groups, 32-channel
        # K chunks per group, 16-row output blocks per group); the GPU launch census checks this
        # restatement against the device
        inst = (groups, x.shape[1] // groups // 32, (co // groups + 15) // 16)
        ok = inst in ((2, 1, 2), (2, 1, 1), (1, 1, 2), (1, 2, 2)) and dilation in (1, 2)
        t.note("g3_launch", ok)
        if not ok:
            raise _lib.AanetError("aanet_conv3x3_grouped_nhwc_f32 failed: unsupported",
                                  _lib.EUNSUPPORTED)
        with t.own():
            y = F.conv2d(x, wsplit, bias, 1, dilation, dilation, groups)
        t.launches.append("aanet_conv3x3_grouped_nhwc_f32")
        return y.contiguous()

    def mdcn_forward_fused(x, offset_mask, weight, bias=None, post_scale=None, post_shift=None,
                           act=None, stride=1, padding=0, dilation=1, deformable_groups=1,
                           mask_scale=2.0, packed_weight=None, groups=1, out=None):
        _check_layout((0,), x, offset_mask, weight, bias, post_scale, post_shift)
        stride, padding, dilation = _int(stride), _int(padding), _int(dilation)
        N, C, H, W = x.shape
        co, cg, kh, kw = weight.shape
        K, dg = kh * kw, deformable_groups
        ho = oracle.out_size(H, kh, stride, padding, dilation)
        wo = oracle.out_size(W, kw, stride, padding, dilation)
        if tuple(offset_mask.shape) != (N, dg * 3 * K, ho, wo):
            raise ValueError(f"offset_mask shape {tuple(offset_mask.shape)} unexpected")
        dtype = np.float64 if x.dtype == torch.float64 else np.float32
        mask = mask_scale * torch.sigmoid(offset_mask[:, 2 * dg * K:])
        y = torch.from_numpy(oracle.mdcn_forward(
            x.contiguous().numpy(), offset_mask[:, :2 * dg * K].contiguous().numpy(),
            mask.contiguous().numpy(), weight.detach().numpy(),
            None if bias is None else bias.detach().numpy(), stride, padding, dilation, groups, dg,
            dtype=dtype))
        if post_scale is not None:
            y = y * post_scale.view(1, -1, 1, 1) + post_shift.view(1, -1, 1, 1)
        t.launches.append("aanet_mdcn_fwd_fused_f32")
        return _act(y, act).contiguous()

    def unreached(name):
        def fn(*a, **k):
            raise AssertionError(f"ops.{name}: no stand-in (the stages were not expected to call it)")
        return fn

    def conv2x_forward(self, x, rem, out_nhwc=False):
        n, k = len(t.launches), len(t.deconv_rem)
        out = real_conv2x(self, x, rem, out_nhwc)
        mine = t.launches[n:]
        if any(t.deconv_rem[k:]):  # the concat went through the deconv's assembly pass
            t.routes += "D" if "aanet_deconv2x_assemble_nhwc_f32" in mine else "d"
        elif "aanet_concat_nhwc_f32" in mine:
            t.routes += "N"
        else:
            t.routes += "C"
        return out

    class CountConvs(torch.utils._python_dispatch.TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            if func is torch.ops.aten.convolution.default and not t._mine:
                t.aten_convs += 1
            return func(*args, **(kwargs or {}))

    real_conv2x = feature.Conv2x.forward
    for mod in (_fuse, deform, feature, refinement, resnet):
        patch(mod, "use_fused", use_fused)
    real_dense = _fuse.dense_grouped_ok
    patch(_fuse, "dense_grouped_ok", lambda conv, x: real_dense(conv, _OnDevice))
    _patch_predicates(t, patch)
    patch(feature.Conv2x, "forward", conv2x_forward)
    for name, fn in (("conv2d_fused", conv2d_fused), ("deconv2x", deconv2x),
                     ("concat_nhwc", concat_nhwc), ("refine_stem", refine_stem),
                     ("disp_warp", disp_warp), ("pack_conv3x3s2", pack_conv3x3s2),
                     ("conv3x3_s2", conv3x3_s2), ("pack_conv3x3_grouped", pack_conv3x3_grouped),
                     ("conv3x3_grouped_nhwc", conv3x3_grouped_nhwc),
                     ("mdcn_forward_fused", mdcn_forward_fused),
                     ("pack_weight_split", lambda w, groups=1: None), ("pack_weight", lambda w: None),
                     ("conv2d_pw", unreached("conv2d_pw")), ("mdcn_pw", unreached("mdcn_pw")),
                     ("resize_bilinear", unreached("resize_bilinear"))):
        patch(ops, name, fn)
    assert warp.ops is ops
    try:
        with CountConvs():
            yield t
    finally:
        for obj, name, value in reversed(saved):
            setattr(obj, name, value)


@functools.lru_cache(maxsize=None)
def cpu_trace(row_id):
    """(Trace, levels as float64 numpy, census dict) of the row's fused path run on the CPU in
    float64, once per row."""
    from aanet_amd._lib import is_nhwc
    row = BY_ID[row_id]
    m = build(row).double()
    x = cast(inputs(row), torch.float64)
    seen = {}
    hooks = []

    def pre(name):
        def hook(mod, args):  # (a hook's return value would replace the input: return None)
            seen.setdefault(name, is_nhwc(args[0]))
        return hook

    def dilated_out(mod, args, out):
        seen.setdefault("dilated_nhwc", is_nhwc(out))

    if row.stage == "GANetFeature":
        hooks.append(m.conv_start[2].register_forward_pre_hook(pre("stem_nhwc")))
    if row.stage == "FeaturePyramidNetwork":
        hooks.append(m.fpn_convs[0].register_forward_pre_hook(pre("fpn_nhwc")))
    if hasattr(m, "dilated_blocks"):
        hooks.append(m.dilated_blocks.register_forward_hook(dilated_out))
    try:
        with fused_on_cpu() as t, torch.no_grad():
            out = levels(m(*x))
    finally:
        for h in hooks:
            h.remove()
    got = dict(halo=t.pred["halo"], s2_conv=t.pred["s2_conv"], deconv2x=t.pred["deconv2x"],
               offset_pack=t.pred["offset_pack"], g3_launch=t.pred["g3_launch"], routes=t.routes,
               stem_fused=("aanet_refine_stem_f32" in t.launches) if has_warp(row) else None,
               resize_skipped=t.resize_skipped, dilated_nhwc=seen.get("dilated_nhwc"),
               fpn_nhwc=seen.get("fpn_nhwc"), stem_nhwc=seen.get("stem_nhwc"),
               out_format=tuple("nhwc" if is_nhwc(o) else "nchw" for o in out),
               aten_convs=t.aten_convs)
    return t, [o.numpy().astype(np.float64) for o in out], got


def census(row):
    """The dispatch columns of the row, evaluated by running the stage's own fast path on the
    CPU (fused_on_cpu) -> a dict with `expect`'s keys."""
    return cpu_trace(row.id)[2]


def expected_launches(row):
    """(entries the fused run must call, entries it must not), from the row's columns.

      conv3x3s2            a conv that conv_bn_act_s2 takes (a T in s2_conv)
      deconv2x_assemble    a Conv2x deconv that leaves the one-pass channels-last route (d)
      .._assemble_nhwc     a Conv2x on the D route
      concat_nhwc          a Conv2x on the N route
      refine_stem          stem_fused
      disp_warp            the stage warps (StereoDRNet / Hourglass refinement)
      conv3x3_grouped      an offset conv reached with NHWC input that has a packing and an
                           instance of the kernel (a T in g3_launch)
      mdcn_fwd_fused       the stage has deformable convs (none of them on a tail kernel)
      conv2d_pw            never; conv2d_fused always (ENTRY_NOT_REQUIRED)"""
    e = row.expect
    on = {
        "aanet_conv3x3s2_f32": "T" in e["s2_conv"],
        "aanet_deconv2x_assemble_f32": "d" in e["routes"],
        "aanet_deconv2x_assemble_nhwc_f32": "D" in e["routes"],
        "aanet_concat_nhwc_f32": "N" in e["routes"],
        "aanet_refine_stem_f32": bool(e["stem_fused"]),
        "aanet_disp_warp_f32": has_warp(row),
        "aanet_conv3x3_grouped_nhwc_f32": "T" in e["g3_launch"],
        "aanet_mdcn_fwd_fused_f32": has_dcn(row),
        "aanet_conv2d_pw_f32": False,
        "aanet_conv2d_fused_f32": True,
    }
    return {k for k, v in on.items() if v}, {k for k, v in on.items() if not v}
