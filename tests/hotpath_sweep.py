"""Case table of the fused eval hot-path sweep (helper, no tests).

The kernels behind AANetHotPath each have edge-shape tests of their own; this table is for the
Python layer that picks them (nets/aggregation.py, nets/_fuse.py, nets/deform.py).  A row is one
whole-path run:

    Row(id, D, sizes, B, kwargs, inter, seed, expect)

  D        cost-volume width at scale 0 (AANetHotPath's max_disp); scale s has D >> s channels
  sizes    explicit per-scale (H, W): nothing here assumes that a pyramid halves exactly
  B        batch
  kwargs   AANetHotPath constructor arguments besides max_disp / no_intermediate_supervision
  inter    intermediate supervision (every fusion has every output branch, one disparity a scale)
  seed     of fill_synthetic(m.aggregation, seed) and synthetic_pyramid_sizes(..., seed)
  expect   the value of every pure dispatch predicate for the row, as LITERALS: a dispatch change
           shows up as a diff of this table (tests/test_hotpath_sweep_cpu.py evaluates them on
           the CPU; `census` below says what each column is)

Feature channels are 32 at every scale.  D is a multiple of 8, or of 4 with one deformable group
(the D/4 offset conv has `deformable_groups` groups).

`expected_launches` turns a row's columns into the C entry points the fused run must and must
not call; tests/test_gpu_hotpath_sweep.py holds the device to it.
"""
import collections
import functools

import numpy as np

FEATURE_CHANNELS = 32

Row = collections.namedtuple("Row", "id D sizes B kwargs inter seed expect")

# The entry points whose presence the dispatch predicates decide.
CENSUS_ENTRIES = ("aanet_conv3x3s2_terms_f32", "aanet_conv3x3s2_f32", "aanet_csa_sum_f32",
                  "aanet_conv3x3_grouped_nhwc_f32", "aanet_mdcn_pw_f32", "aanet_conv2d_pw_f32",
                  "aanet_mdcn_fwd_fused_f32")


def _x(epilogue, s2_sums, s2_conv, heads, halo, post, split_bytes, pipeline, offset_g3,
       dense_grouped):
    # one value for (first fusion, later fusions) where they agree
    epilogue = epilogue if isinstance(epilogue, tuple) else (epilogue, epilogue)
    s2_sums = s2_sums if isinstance(s2_sums, tuple) else (s2_sums, s2_sums)
    post = post if isinstance(post, tuple) else (post, post)
    return dict(epilogue=epilogue, s2_sums=s2_sums, s2_conv=s2_conv, heads=heads, halo=halo,
                post=post, split_bytes=split_bytes, pipeline=pipeline, offset_g3=offset_g3,
                dense_grouped=dense_grouped)


T, F = True, False
_C3 = [(16, 40), (8, 20), (4, 10)]       # halves exactly, every width a multiple of 4 at scale 0
_ODD = [(13, 37), (7, 19), (4, 10)]      # odd, ceil-halved: the down convs' own output sizes
_S28 = [(12, 28), (6, 14), (3, 7)]

# expect columns, in _x order (epilogue and s2_sums: on the volumes for the first fusion, and
# on its outputs for the later ones -- an output branch has the size of its down term from scale
# 0, the ceil-halved one, whatever the volume's was):
#   epilogue  s2_sums  s2_conv (1,0) (2,0)a (2,0)b (2,1)  heads (one launch)  halo
#   post (conv1 stage, final stage)  split_bytes  pipeline  offset_g3 and dense_grouped per scale
_D64 = dict(s2_conv=(T, T, T, T), heads=T, halo=T, post=(T, T), split_bytes=40960,
            offset_g3=(T, F, F), dense_grouped=(F, T, F))


def _d64(epilogue, s2_sums, pipeline, **over):
    return _x(**{**_D64, "epilogue": epilogue, "s2_sums": s2_sums, "pipeline": pipeline, **over})


ROWS = [
    Row("d64_exact", 64, _C3, 2, {}, F, 41, _d64(T, T, T)),
    Row("d64_w42", 64, [(16, 42), (8, 21), (4, 11)], 1, {}, F, 42, _d64(F, T, F)),
    Row("d64_odd_ceil", 64, _ODD, 2, {}, F, 43, _d64(F, T, F)),
    # floor-halved: the coarse volumes are not the down convs' output sizes, so the first fusion
    # resizes the same-scale terms and the stride-2 kernels cannot sum them; its outputs are
    # ceil-halved, so the later fusions' can
    Row("d64_odd_floor", 64, [(13, 36), (6, 18), (3, 9)], 2, {}, F, 44, _d64(F, (F, T), F)),
    Row("d64_one_row", 64, [(3, 132), (2, 66), (1, 33)], 1, {}, F, 45, _d64(F, T, F)),
    Row("d64_tiny", 64, [(5, 9), (3, 5), (2, 3)], 1, {}, F, 46, _d64(F, T, F)),
    Row("d64_inter_17x44", 64, [(17, 44), (9, 22), (5, 11)], 3, {}, T, 47, _d64(F, T, F)),
    Row("d64_inter_24x52", 64, [(24, 52), (12, 26), (6, 13)], 2, {}, T, 48, _d64(T, T, T)),
    Row("d64_two_scales", 64, _C3[:2], 2, dict(num_scales=2), F, 49,
        _d64(T, F, F, s2_conv=(T,), offset_g3=(T, F), dense_grouped=(F, T))),
    # two scales: one 2x term, so W % 4 is all that refuses the epilogue (with three scales an
    # exact 4x term implies it)
    Row("d64_two_scales_w42", 64, [(16, 42), (8, 21)], 1, dict(num_scales=2), F, 64,
        _d64(F, F, F, s2_conv=(T,), offset_g3=(T, F), dense_grouped=(F, T))),
    Row("d64_f3_db1", 64, _ODD, 1, dict(num_fusions=3, num_deform_blocks=1), F, 50,
        _d64(F, T, F)),
    Row("d64_no_deform", 64, _C3, 1, dict(num_deform_blocks=0), F, 51,
        _d64(T, T, T, offset_g3=None, dense_grouped=None)),
    Row("d64_dg1", 64, _S28, 1, dict(deformable_groups=1), F, 52,
        _d64(T, T, T, offset_g3=(T, T, F), dense_grouped=(F, F, F))),
    Row("d64_dil1", 64, _S28, 1, dict(mdconv_dilation=1), F, 53, _d64(T, T, T)),
    Row("d64_two_blocks", 64, _S28, 2, dict(num_stage_blocks=2), F, 54,
        _d64(T, T, F, post=(F, T))),
    Row("d16_w42", 16, [(16, 42), (8, 21), (4, 11)], 2, {}, F, 55,
        _x(F, F, (F, F, F, F), F, F, F, 0, F, (F, F, F), (F, F, F))),
    Row("d24_coarse_w10", 24, [(12, 40), (6, 20), (3, 10)], 2, {}, F, 56,
        _x(T, F, (F, F, F, F), F, F, F, 0, F, (F, F, F), (F, F, F))),
    Row("d24_two_blocks_inter", 24, [(11, 30), (6, 15), (3, 8)], 1, dict(num_stage_blocks=2), T,
        57, _x(F, F, (F, F, F, F), F, F, F, 0, F, (F, F, F), (F, F, F))),
    Row("d32_tiny", 32, [(5, 9), (3, 5), (2, 3)], 3, {}, F, 58,
        _x(F, F, (T, T, F, F), T, T, F, 16384, F, (F, F, F), (T, F, F))),
    Row("d32_all_deform", 32, _ODD, 1, dict(num_deform_blocks=6), F, 59,
        _x(F, F, (T, T, F, F), T, None, F, 16384, F, (F, F, F), (T, F, F))),
    Row("d40_inter", 40, _C3, 2, {}, T, 60,
        _x(T, F, (F, F, F, F), F, F, F, 0, F, (F, F, F), (F, F, F))),
    Row("d48_inter", 48, [(12, 40), (6, 20), (3, 10)], 2, {}, T, 61,
        _x(T, F, (F, F, F, F), F, F, F, 33792, F, (F, F, F), (F, F, F))),
    Row("d96_heads", 96, _ODD, 2, {}, F, 62,
        _x(F, F, (T, T, F, F), F, T, F, 110592, F, (F, F, F), (T, F, F))),
    Row("d128_inter", 128, [(9, 24), (5, 12), (3, 6)], 1, {}, T, 63,
        _x(F, F, (T, F, T, T), F, T, F, 163840, F, (T, T, F), (F, F, T))),
]
BY_ID = {r.id: r for r in ROWS}
assert len(BY_ID) == len(ROWS)

# Predicates (columns of `expect`) that cannot take both values inside the table's legal range
# ({column: reason}); every other column must be true in one row and false in another.
NOT_REQUIRED = {}


def num_scales(row):
    return row.kwargs.get("num_scales", 3)


def num_fusions(row):
    return row.kwargs.get("num_fusions", 6)


def num_deform_blocks(row):
    return row.kwargs.get("num_deform_blocks", 3)


def volume_shapes(row):
    return [(row.B, row.D >> s, h, w) for s, (h, w) in enumerate(row.sizes)]


def output_shapes(row):
    """The shapes a fusion with every output branch hands to the next: branch i has the size of
    its down term from scale 0 (nets/aggregation.py:388-400), i.e. scale 0's ceil-halved i times."""
    h, w = row.sizes[0]
    out = []
    for s in range(num_scales(row)):
        out.append((row.B, row.D >> s, h, w))
        h, w = (h + 1) // 2, (w + 1) // 2
    return out


def build_model(row):
    """(AANetHotPath in eval mode on the CPU with the row's synthetic weights, its aggregation
    state dict as numpy arrays)."""
    from aanet_amd import nets
    from tests.golden_io import fill_synthetic
    m = nets.AANetHotPath(row.D, no_intermediate_supervision=not row.inter, **row.kwargs)
    fill_synthetic(m.aggregation, row.seed)
    sd = {k: v.numpy().copy() for k, v in m.aggregation.state_dict().items()}
    return m.eval(), sd


def inputs(row):
    from tests.golden_io import synthetic_pyramid_sizes
    return synthetic_pyramid_sizes(row.B, FEATURE_CHANNELS, row.sizes, row.seed)


def oracle_kwargs(row):
    return dict(num_scales=num_scales(row), num_fusions=num_fusions(row),
                num_deform_blocks=num_deform_blocks(row), intermediate_supervision=row.inter,
                dilation=row.kwargs.get("mdconv_dilation", 2),
                dg=row.kwargs.get("deformable_groups", 2),
                num_stage_blocks=row.kwargs.get("num_stage_blocks", 1))


@functools.lru_cache(maxsize=None)
def oracle_reference(row_id):
    """The CPU oracle on the row, computed once and shared (callers leave it unchanged):
    {"disp64", "agg64": float64 disparities (coarse to fine, as the model returns them) and
    aggregated volumes (scale order); "disp32", "agg32": the oracle's own float32 run}."""
    from oracle import aggregation as oagg
    row = BY_ID[row_id]
    _, sd = build_model(row)
    left, right = inputs(row)
    ln, rn = [t.numpy() for t in left], [t.numpy() for t in right]
    out = {}
    for tag, dtype in (("64", np.float64), ("32", np.float32)):
        disps, aggs = oagg.hot_path(ln, rn, sd, row.D, dtype=dtype, with_aggregation=True,
                                    **oracle_kwargs(row))
        out["disp" + tag], out["agg" + tag] = disps, aggs
    return out


def own_error(row_id):
    """(aggregated cost relative to max|ref|, disparity px): the float32 oracle's distance to the
    float64 one, each at its worst level."""
    r = oracle_reference(row_id)
    agg = max(np.abs(a - b).max() / np.abs(b).max() for a, b in zip(r["agg32"], r["agg64"]))
    disp = max(np.abs(a - b).max() for a, b in zip(r["disp32"], r["disp64"]))
    return float(agg), float(disp)


class _SplitPack:
    _aanet_split = True


class Vol:
    """Stand-in for a cost volume on the GPU: the dispatch predicates read only these."""
    is_cuda = True

    def __init__(self, shape):
        import torch
        self.shape = torch.Size(shape)


def census(row, m, grouped_pack_bytes):
    """The pure dispatch predicates on the row's shapes -> a dict with `expect`'s keys.

      epilogue       csa_epilogue_ok(scale 0, the coarse scales): (on the volumes, on
                     output_shapes -- what the fusions after the first see)
      s2_sums        (fusions[0]._s2_sums_ok(volumes), fusions[1]._s2_sums_ok(output_shapes))
      s2_conv        s2_conv_ok of every conv of fusions[0]'s down chains, in (i, j, k) order
      heads          fusions[0]._down0_heads takes the one-launch form: every head conv on the
                     stride-2 kernel and at most 96 output channels together (the device packer
                     and the launch stubbed)
      halo           halo_input_ok(conv2, width) of fusions[0]'s scale-0 SimpleBottleneck
                     (None: the block is deformable)
      post           _post_for offers a stage (the (64, 64, 1, 1) weight test and the block
                     tests; a split packing stands in for the device packer): (the first
                     fusion's tail: the second's conv1; the last fusion's tail with `regress`:
                     final_conv + soft-argmin)
      split_bytes    aanet_conv_weight_pack_split_bytes of that D -> D 1x1 weight
      pipeline       _pipeline_ok(volumes, fused=True) with the `pipeline` option set
      offset_g3      per scale: offset_conv_pack of the last fusion's offset conv finds a packing
                     (grouped_pack_bytes(co, c, groups) stands in for the device packer)
      dense_grouped  per scale: dense_grouped_ok of the same conv
    (the last two None when the model has no deformable block)."""
    from aanet_amd import _lib, ops
    from aanet_amd.nets import _fuse, aggregation
    from aanet_amd.nets.aggregation import csa_epilogue_ok
    from aanet_amd.nets.deform import SimpleBottleneck
    agg = m.aggregation
    vols = [Vol(s) for s in volume_shapes(row)]
    f0, fl = agg.fusions[0], agg.fusions[-1]
    later = [Vol(s) for s in output_shapes(row)]
    got = {"epilogue": (csa_epilogue_ok(vols[0], vols[1:]), csa_epilogue_ok(later[0], later[1:])),
           "s2_sums": (f0._s2_sums_ok(vols), agg.fusions[1]._s2_sums_ok(later))}
    got["s2_conv"] = tuple(_fuse.s2_conv_ok(layer[0])
                           for i in range(1, len(f0.fuse_layers)) for j in range(i)
                           for layer in f0.fuse_layers[i][j])
    real = ops.pack_conv3x3s2, ops.conv3x3_s2
    ops.pack_conv3x3s2 = lambda w: object()
    ops.conv3x3_s2 = lambda x, wsplit, bias, co, co_a, *a, **k: ("a", "b" if co_a < co else None)
    try:
        import torch
        got["heads"] = bool(f0._down0_heads(torch.empty(volume_shapes(row)[0])))
    finally:
        ops.pack_conv3x3s2, ops.conv3x3_s2 = real
    b0 = f0.branches[0][0]
    got["halo"] = _fuse.halo_input_ok(b0.conv2, b0.conv1.weight.shape[0]) \
        if isinstance(b0, SimpleBottleneck) else None
    real = aggregation.folded
    aggregation.folded = lambda conv, bn: (conv.weight, None, _SplitPack())
    try:
        got["post"] = (agg._post_for(0, False) is not None,
                       agg._post_for(num_fusions(row) - 1, True) is not None)
    finally:
        aggregation.folded = real
    got["split_bytes"] = int(_lib.lib().aanet_conv_weight_pack_split_bytes(row.D, row.D, 1, 1, 1))
    agg.set_options(pipeline=True)
    try:
        got["pipeline"] = agg._pipeline_ok(vols, True)
    finally:
        agg.set_options(pipeline=False)
    if num_deform_blocks(row) == 0:
        got["offset_g3"] = got["dense_grouped"] = None
        return got
    convs = [fl.branches[s][0].conv2.offset_conv for s in range(num_scales(row))]
    real = ops.pack_conv3x3_grouped
    ops.pack_conv3x3_grouped = \
        lambda w, g: grouped_pack_bytes(w.shape[0], w.shape[1] * g, g) or None
    try:
        got["offset_g3"] = tuple(_fuse.offset_conv_pack(c) is not None for c in convs)
    finally:
        ops.pack_conv3x3_grouped = real
    got["dense_grouped"] = tuple(_fuse.dense_grouped_ok(c, v) for c, v in zip(convs, vols))
    return got


def expected_launches(row):
    """(entries the fused run must call, entries it must not), from the row's columns.

    A fusion with more than one output branch exists in every row (S >= 2, at least 3 fusions).
      conv3x3s2_terms   the stride-2 sums: s2_sums in some fusion
      conv3x3s2         the down chains conv by conv or as the heads launch: a fusion without
                        s2_sums, and a down conv the kernel takes
      csa_sum           every branch that no other kernel sums: absent only when in every fusion
                        the scale-0 tail takes branch 0 (epilogue, and a tail kernel at scale 0:
                        width <= 64) and the stride-2 kernels take the coarse ones
      conv3x3_grouped   a deformable block whose offset conv has a packing
      mdcn_pw           a deformable block on a tail kernel (every D here: scale 1 is <= 64 wide)
      conv2d_pw         a plain block (fewer deformable fusions than fusions)
      mdcn_fwd_fused    a deformable block past the tail kernels (scale-0 width > 64)"""
    e = row.expect
    deform = num_deform_blocks(row) > 0
    on = {
        "aanet_conv3x3s2_terms_f32": any(e["s2_sums"]),
        "aanet_conv3x3s2_f32": not all(e["s2_sums"]) and any(e["s2_conv"]),
        "aanet_csa_sum_f32": not (all(e["epilogue"]) and row.D <= 64 and all(e["s2_sums"])),
        "aanet_conv3x3_grouped_nhwc_f32": deform and any(e["offset_g3"]),
        "aanet_mdcn_pw_f32": deform,
        "aanet_conv2d_pw_f32": num_deform_blocks(row) < num_fusions(row),
        "aanet_mdcn_fwd_fused_f32": deform and row.D > 64,
    }
    return {k for k, v in on.items() if v}, {k for k, v in on.items() if not v}
